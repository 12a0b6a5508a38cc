"""The geometries of test_conv3d_tile_edges.py: one table for every contraction that runs through the 128 x 64 x 32 implicit-GEMM
tile of csrc/bnn_conv3d_tile.hpp (K7, K9, K11, K17, K19), each case at an edge of the tile's own decode, with the properties it
is in the table for.  test_table_claims asserts the properties (on the CPU, with torch), so that an edit cannot lose an edge."""
import numpy as np

BM, BN, BK = 128, 64, 32            # C3_BM, C3_BN, C3_BK: rows, columns and reduction elements of one tile


class Geometry:
    """B images (C, *vol) -> O channels; kernel, stride, padding, dilation as triples."""

    def __init__(self, B, C, vol, O, kernel, stride=1, padding=0, dilation=1, groups=1):
        tri = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * 3         # noqa: E731
        self.B, self.C, self.vol, self.O, self.groups = B, C, tuple(vol), O, groups
        self.kernel, self.stride, self.padding, self.dilation = tri(kernel), tri(stride), tri(padding), tri(dilation)
        self.out = tuple((self.vol[i] + 2 * self.padding[i] - self.dilation[i] * (self.kernel[i] - 1) - 1) // self.stride[i] + 1
                         for i in range(3))
        self.Cg, self.Ng = C // groups, O // groups
        self.T = int(np.prod(self.kernel))
        self.K = self.Cg * self.T
        self.P, self.Pin = int(np.prod(self.out)), int(np.prod(self.vol))

    @property
    def x_shape(self):
        return (self.B, self.C) + self.vol

    @property
    def w_shape(self):
        return (self.O, self.Cg) + self.kernel

    @property
    def geo(self):
        return self.stride, self.padding, self.dilation, self.groups

    @property
    def lrt_args(self):
        """test_lrt_conv_device.Case's arguments"""
        return (self.B, self.C, self.vol, self.O, self.kernel, self.stride, self.padding, self.dilation, self.groups)

    @property
    def moment_spec(self):
        """test_moment_conv.CASES' tuple, with a bias"""
        return (self.x_shape, self.O, self.kernel, self.stride, self.padding, self.dilation, self.groups, True)


# name -> (geometry, claims).  Claims: P4 = P % 4; padding_only / unreached = output / input positions per channel of one image
# that read only padding / that no tap reaches; the rest are asserted from the geometry itself (test_table_claims).
TABLE = {
    # Cg = Ng = 70: a partial second column block in FWD, DGRAD and WGRAD; K = 140: a partial second row block in WGRAD
    "wide": (Geometry(2, 70, (3, 4, 5), 70, (1, 2, 1)), dict(Cg=70, Ng=70, K=140, P=45, P4=1, padding_only=0, unreached=0)),
    # the same with the group offset; B P = 27: one k-tile
    "wide-groups": (Geometry(3, 132, (2, 3, 3), 140, (2, 1, 1), groups=2),
                    dict(Cg=66, Ng=70, K=132, P=9, P4=1, BP=27, padding_only=0, unreached=0)),
    # every per-axis value differs from the other two
    "peraxis": (Geometry(3, 5, (5, 7, 9), 7, (2, 3, 1), (1, 2, 3), (2, 0, 1), (3, 1, 2)),
                dict(out=(6, 3, 4), P=72, P4=0, padding_only=18, unreached=210)),
    # a second assignment of the axes, with groups
    "peraxis-odd": (Geometry(2, 6, (4, 9, 7), 10, (1, 3, 2), (3, 1, 2), (0, 2, 1), (1, 3, 2), 2),
                    dict(out=(2, 7, 4), P=56, P4=0, padding_only=0, unreached=198)),
    # padding at least as large as the window: 48 of 72 output positions read nothing; M = B P = 144 > B Pin = 36
    "padding-only": (Geometry(2, 3, (2, 3, 3), 5, (1, 2, 1), 1, (1, 2, 0)), dict(P=72, P4=0, padding_only=48, unreached=0)),
    # stride larger than the window, and an unread tail: 90 of 144 input positions get gradient exactly 0
    "unreached": (Geometry(2, 4, (6, 8, 3), 6, (1, 2, 1), (2, 3, 1)), dict(P=27, P4=3, Pin=144, padding_only=0, unreached=90)),
    # stride equals dilation: one parity class of inputs is reached
    "stride-eq-dil": (Geometry(2, 3, (6, 7, 5), 4, 3, 2, 2, 2), dict(K=81, P=36, P4=0, padding_only=0, unreached=174)),
    # P = 1: FastDiv by 1 for OW, OH and P; M = 130 rows from 130 images: two row blocks, every quad spans four images
    "one-output": (Geometry(130, 3, (2, 2, 2), 5, 2), dict(P=1, P4=1, padding_only=0, unreached=0)),
    # P = Pin = T = 1
    "point": (Geometry(5, 2, (1, 1, 1), 3, 1), dict(P=1, P4=1, Pin=1, T=1, K=2, padding_only=0, unreached=0)),
    # B P = 16 <= 32: K7 writes the weight gradient with no slab; P = 8: the vector-store path
    "one-ktile": (Geometry(2, 3, (3, 3, 3), 4, 2), dict(P=8, P4=0, BP=16, padding_only=0, unreached=0)),
    # B P = 750: 24 k-tiles in 12 slabs of two, the last slab short, its last k-tile partial, image boundaries off the k-tile grid
    "long-reduction": (Geometry(5, 2, (5, 5, 5), 3, (2, 1, 1), 1, (1, 0, 0)),
                       dict(P=150, P4=2, BP=750, padding_only=0, unreached=0)),
}

CASES = list(TABLE)
# the cases that run S = 3 with a shared and with a per-sample input through K7 and K9 (S = 1 elsewhere)
MULTI_SAMPLE = ("wide", "wide-groups", "peraxis", "one-output")
# DGRAD stores exact zeros at the input positions no tap reaches
EXACT_ZERO = ("unreached", "stride-eq-dil", "peraxis", "peraxis-odd")


def geometry(name):
    return TABLE[name][0]
