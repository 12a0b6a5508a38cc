"""The environment knobs of the C side (csrc/bnn_knobs.hpp).  The production library reads two -- BNN_DENSE_TILE and
BNN_DRAW_LEAN, each of which selects a second correct kernel -- and holds neither the name of any diagnostic knob (phase skips
that make a kernel compute wrong results, stamp buffers written through a raw device address from the environment, A/B
switches) nor a kernel instantiation only such a knob launches; those live in the diagnostic library (make diag, -DBNN_DIAG).

Every check here fails on the commit before the header: getenv in bnn_dense / bnn_gemm / bnn_linear / bnn_linear_bwd.hip (20
reads), all 17 names below in the library, 92 of 154 k_dense_bf16 instantiations with DIAG != 0, 3 k_linear_sym with STAMPS, the
one-role k_wgrad_bf16_dma, and k_draw_multi<1 / 2 / 4 / 8>.

CPU only.  Kernel names are read as mangled: the template arguments of a kernel are its run of L<i|b><value>E literals."""
import glob
import os
import re

from test_dense_coresident import _code_object_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesianneuralnetworks_amd", "csrc")

PRODUCTION_KNOBS = ["BNN_DENSE_TILE", "BNN_DRAW_LEAN"]
# read by the diagnostic library only ...
DIAG_KNOBS = ["BNN_DENSE_DIAG", "BNN_DENSE_STAMPS", "BNN_CONV_DIAG", "BNN_WGRAD_DIAG", "BNN_WGRAD_NOEPS", "BNN_STAMPS",
              "BNN_DENSE_XCD", "BNN_DRAW_TAPG", "BNN_DRAW_KL_ITEMS", "BNN_DRAW_SPLIT", "BNN_XCD_A", "BNN_LINEAR_KERNEL"]
# ... and deleted with the code only they reached
DELETED_KNOBS = ["BNN_DRAW_UNROLL", "BNN_DENSE_LOADER_PRIO", "BNN_WGRAD_ROLES", "BNN_F32_MFMA", "BNN_TILE"]


def test_getenv_only_in_the_knobs_header():
    files = [f for f in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(f) and not f.endswith(".o")]    # sources, not objects
    assert len(files) > 30
    readers = sorted(os.path.basename(f) for f in files if "getenv" in open(f, errors="replace").read())
    assert readers == ["bnn_knobs.hpp"], readers
    header = open(os.path.join(CSRC, "bnn_knobs.hpp")).read()
    for name in PRODUCTION_KNOBS + DIAG_KNOBS:
        assert '"%s"' % name in header, name
    for name in DELETED_KNOBS:
        assert name not in header, name


def test_production_library_holds_two_knob_names():
    blob = open(os.path.join(ROOT, "bayesianneuralnetworks_amd", "libbnn_hip.so"), "rb").read()
    for name in PRODUCTION_KNOBS:
        assert name.encode() + b"\0" in blob, name
    found = [name for name in DIAG_KNOBS + DELETED_KNOBS if name.encode() + b"\0" in blob]
    assert found == [], found
    assert b"diagnostic build (BNN_DIAG)" not in blob


def _template_args(name, kernel):
    """The integral template arguments of mangled kernel `name` if it is an instantiation of bnn::<kernel>, else None."""
    m = re.match(r"_ZN3bnn%d%sI((?:L[a-z]n?\d+E)+)E" % (len(kernel), kernel), name)
    if not m:
        return None
    return [-int(v[1:]) if v.startswith("n") else int(v) for v in re.findall(r"L[a-z](n?\d+)E", m.group(1))]


def test_template_args_reads_mangled_names():
    assert _template_args("_ZN3bnn12k_dense_bf16ILi4ELi5ELi2ELi2ELi2ELi1ELb1ELi6ELb0EEEvNS_11DenseParamsE", "k_dense_bf16") == \
        [4, 5, 2, 2, 2, 1, 1, 6, 0]
    assert _template_args("_ZN3bnn12k_draw_multiILi8EEEvNS_10DrawLaunchE", "k_draw_multi") == [8]
    assert _template_args("_ZN3bnn12k_draw_multiENS_10DrawLaunchE", "k_draw_multi") is None
    assert _template_args("_ZN3bnn11k_draw_leanENS_10DrawLaunchE", "k_draw_multi") is None


def test_production_code_objects_hold_no_diagnostic_kernel():
    kernels = _code_object_kernels(os.path.join(ROOT, "bayesianneuralnetworks_amd", "libbnn_hip.so"))
    dense = {n: _template_args(n, "k_dense_bf16") for n in kernels if _template_args(n, "k_dense_bf16")}
    sym = {n: _template_args(n, "k_linear_sym") for n in kernels if _template_args(n, "k_linear_sym")}
    assert len(dense) > 20 and len(sym) > 10                                     # the parser sees the families
    assert all(len(a) == 9 for a in dense.values()) and all(len(a) == 10 for a in sym.values())
    # <TM, TN, NWM, NWN, ST, YM, RELU, DIAG, DROP>
    assert sorted(n for n, a in dense.items() if a[7] != 0) == []
    # <NW, RW, BN, CH, S, NB, B_MODE, COMPUTE, ABF, STAMPS>
    assert sorted(n for n, a in sym.items() if a[9] != 0) == []
    # the one-role weight-gradient kernel is gone; the two-role one is the hot path
    wgrad_dma = sorted(n for n in kernels if re.match(r"_ZN3bnn\d+k_wgrad_bf16_dma", n))
    assert wgrad_dma == ["_ZN3bnn17k_wgrad_bf16_dma8ENS_11WgradParamsE"], wgrad_dma
    # one full draw kernel and one lean one: no unrolled instantiations
    draws = sorted(n for n in kernels if re.match(r"_ZN3bnn\d+k_draw_(multi|lean)", n))
    assert draws == ["_ZN3bnn11k_draw_leanENS_10DrawLaunchE", "_ZN3bnn12k_draw_multiENS_10DrawLaunchE"], draws
