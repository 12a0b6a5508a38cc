"""The co-resident instantiation of the dense kernel (csrc/bnn_dense.hip, k_dense_bf16<4, 5, 2, 2, 2, ...>): the 128 x 160 tile
on a 2-stage ring, two workgroups per CU, taken by plain bf16 launches of tile 1.

CPU: its code objects fit two 512-thread workgroups on a CU -- LDS <= 80 KiB, <= 128 VGPR + AGPR per lane (4 waves per SIMD),
no scratch, no spills.
GPU: it gives the bits of the one-workgroup-per-CU kernel (BNN_DENSE_TILE=5, in a fresh process; BNN_DENSE_TILE=1 forces the
co-resident one in another) on the BASELINE layer shapes -- ReLU with bf16 output, fp32 output, the fused classifier head at
S = 1, 8, 17 -- and on ragged M / N / K."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CO_PREFIX = "_ZN3bnn12k_dense_bf16ILi4ELi5ELi2ELi2ELi2E"     # <TM = 4, TN = 5, NWM = 2, NWN = 2, ST = 2, ...>


def _code_object_kernels(lib_path=None):
    """name -> metadata fields of every kernel in the gfx950 code objects of a built library (default: the loaded one)."""
    from bayesianneuralnetworks_amd import _lib
    lib_path = lib_path or _lib.LIB_PATH
    llvm = "/opt/rocm/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm LLVM tools not found")
    notes = ""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([tools[0], "--dump-section=.hip_fatbin=" + fat, lib_path, os.path.join(d, "lib.so")])
        blob = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]      # one bundle per translation unit
        for i, a in enumerate(starts):
            part, co = os.path.join(d, "b%d.bin" % i), os.path.join(d, "b%d.co" % i)
            open(part, "wb").write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.check_call([tools[1], "--unbundle", "--type=o", "--input=" + part,
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
            notes += subprocess.check_output([tools[2], "--notes", co]).decode()
    kernels = {}
    for block in notes.split("- .agpr_count")[1:]:
        fields = dict(re.findall(r"\.(name|vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                                 r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\S+)", block))
        fields["agpr_count"] = block.split("\n", 1)[0].strip(" :")
        if "name" in fields:
            kernels[fields["name"]] = fields
    return kernels


DIAG_LIB = os.path.join(ROOT, "bayesianneuralnetworks_amd", "libbnn_hip_diag.so")     # make -C csrc diag; not built by build()


@pytest.mark.parametrize("build", ["production", "diagnostic"])
def test_coresident_code_objects_fit_two_workgroups_per_cu(build):
    if build == "diagnostic" and not os.path.exists(DIAG_LIB):
        pytest.skip("diagnostic library not built")
    kernels = _code_object_kernels(DIAG_LIB if build == "diagnostic" else None)
    co = {n: f for n, f in kernels.items() if n.startswith(CO_PREFIX)}
    # ReLU or not x {bf16, fp32, fused head} = 6 (dense_launch, BNN_DENSE_CO: three launches per ReLU setting); the diagnostic
    # library adds the stamped bf16 build (BNN_DENSE_DIAG=6) of each ReLU setting: 2 x 4 = 8
    assert len(co) == (8 if build == "diagnostic" else 6), sorted(co)
    for n, f in co.items():
        assert int(f["max_flat_workgroup_size"]) == 512, (n, f)
        assert int(f["group_segment_fixed_size"]) <= 80 * 1024, (n, f)              # two workgroups in the CU's 160 KiB
        regs = int(f["vgpr_count"]) + int(f["agpr_count"])
        assert (regs + 7) // 8 * 8 <= 128, (n, f)                                   # 4 waves per SIMD = two 8-wave workgroups
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0, (n, f)
        assert int(f["private_segment_fixed_size"]) == 0, (n, f)


# ------------------------------------------------------------------------------------------------ GPU: bits of the old kernel
# name, S, M, N, K, shared x, relu, output (bf16 / f32 / head: Nh outputs)
CASES = [
    ("layer1", 8, 512, 1200, 784, True, True, "bf16"),         # the BASELINE step's layer 1 (input shared by the samples)
    ("layer2_f32", 8, 512, 1200, 1200, False, False, "f32"),
    ("head_s1", 1, 512, 1200, 1200, False, True, 10),          # layer 2 + the classifier head, as the step runs it
    ("head_s8", 8, 512, 1200, 1200, False, True, 10),
    ("head_s17", 17, 512, 1200, 1200, False, True, 10),
    ("ragged_bf16", 3, 130, 200, 72, False, True, "bf16"),     # N = 1.25 panels, M tail, two k-steps, the second a K tail
    ("ragged_f32", 2, 70, 240, 328, True, False, "f32"),
    ("ragged_head", 2, 261, 168, 200, False, False, 7),
    ("one_kstep_bf16", 2, 100, 160, 48, False, True, "bf16"),  # K <= 64: the main loop never runs, only the peeled step
    ("one_kstep_f32", 3, 37, 88, 64, True, False, "f32"),
    ("one_kstep_head", 3, 64, 240, 64, True, True, 5),
]


def _run_cases(out_path):
    """Every case of CASES on seeded posteriors and inputs; each output saved as raw bits."""
    import torch
    import seeded
    from bayesianneuralnetworks_amd import _lib, ops
    from bayesianneuralnetworks_amd._rng import DrawKey
    dev = torch.device("cuda:0")
    blobs = {}
    for ci, (name, S, M, N, K, shared, relu, out) in enumerate(CASES):
        gen = torch.Generator().manual_seed(700 + ci)
        hid = [t.to(dev) for t in seeded.posterior(gen, (N, K), True)]
        layers = [(*hid, DrawKey(9, 2 * ci + 1, 0, S, 3, gen=1), DrawKey(9, 2 * ci + 2, 0, S, 3, gen=1))]
        if not isinstance(out, str):
            head = [t.to(dev) for t in seeded.posterior(gen, (out, N), True)]
            layers.append((*head, DrawKey(9, 101 + 2 * ci, 0, S, 3, gen=1), DrawKey(9, 102 + 2 * ci, 0, S, 3, gen=1)))
        pre = ops.draw_layers(layers, S)
        x = torch.randn((M, K) if shared else (S, M, K), generator=gen).to(dev).bfloat16()
        xs = 0 if shared else M * K
        if out == "bf16":
            y = ops._dense_raw(x, xs, M, pre[0], K, relu, torch.bfloat16, pad_rows=True)
            blobs[name] = y.contiguous().view(torch.int16).cpu().numpy()
        elif out == "f32":
            y = ops._dense_raw(x, xs, M, pre[0], K, relu, torch.float32)
            blobs[name] = y.contiguous().view(torch.int32).cpu().numpy()
        else:
            hp = ops._dense_head_raw(x, xs, M, pre[0], K, relu, pre[1])
            blobs[name] = hp.p.contiguous().view(torch.int32).cpu().numpy()
    torch.cuda.synchronize()
    _lib.check_device(dev)
    np.savez(out_path, **blobs)


def _in_fresh_process(tile, path):
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_dense_coresident as t; t._run_cases(%r)"
            % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), path))
    env = dict(os.environ, BNN_DENSE_TILE=str(tile))
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=600, cwd=ROOT)
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
def test_coresident_equals_one_workgroup_per_cu_bit_for_bit(tmp_path):
    new = _in_fresh_process(1, str(tmp_path / "coresident.npz"))
    old = _in_fresh_process(5, str(tmp_path / "one_per_cu.npz"))
    assert sorted(new) == sorted(old) == sorted(c[0] for c in CASES)
    for k in old:
        assert new[k].shape == old[k].shape, k
        assert np.array_equal(new[k], old[k]), (k, int((new[k] != old[k]).sum()))
