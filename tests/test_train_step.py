"""The backward of a training step, layer by layer, against tests/golden/bwdref.py: every parameter gradient and every
inter-layer input gradient of a real `loss.backward()` over NormalLinear layers (bf16 compute with bf16 hidden activations, a
fused ReLU, the KL gradient fused into the weight-gradient launches, a narrow head, a shared input) held to a DERIVED
per-element bound around a float64 evaluation of the operands each layer actually consumed (teacher forcing).  bwdref's
docstring lists the rounding points and derives the bound.

CPU: an fp32 torch emulation of each kernel (rounded operands, fp32 matmul, the epilogue in fp32) stands in for the device on the
smallest configuration.  It must lie inside the bound with zero violations, and each of a list of wrong kernels (a dropped
batch row, a mispaired sample, a shifted Philox block, a misplaced dsoftplus, ...) must leave it.
GPU: the configurations below, chosen as the smallest shapes that reach each dispatch branch of
bnn_linear_backward_weight_sampled, bnn_linear_backward_narrow_sampled and ops._SampledLinear.backward.
Host: the two argument checks of bnn_linear_backward_narrow_sampled that come before its launch.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import bwdref
import seeded
from bayesianneuralnetworks_amd import _lib

gpu = pytest.mark.gpu
N_BATCHES = 7
KL_C = 2.5e5            # the KL term's weight in the loss: its gradient is then within a few orders of the likelihood's everywhere
PRIOR = (0.0, 0.1)
RECORD_DIR_ENV = "BNN_TEST_RECORD_DIR"      # a directory: the GPU test appends its worst |err| / bound ratios to train_step_check.jsonl there
WS_SLAB_BYTES = (4 << 20) - (64 << 10)      # _lib.ensure_workspace's 4 MiB less the ticket area (kTicketBytes, csrc/bnn_gemm.hip)


# =================================================================================================== what runs where
def layer_plan(dims, S, mode, x_bf16):
    """Per layer, the kernels ops._SampledLinear.backward and the two host functions choose (their conditions restated), as the
    `spec` bwdref reads plus the names and the launch count of the layer's backward."""
    L = len(dims) - 1
    xdt = []                                  # dtype of each layer's saved input
    for i in range(L):
        if i == 0:
            xdt.append("bf16" if x_bf16 else "f32")
        else:                                 # nn.fuse_activations: a fused-ReLU producer emits bf16 for a consumer with K % 8 == 0
            xdt.append("bf16" if (mode == "bf16" and dims[i] % 8 == 0) else "f32")
    plan = []
    for i in range(L):
        K, N = dims[i], dims[i + 1]
        shared = S == 1 or i == 0
        need_gx = i > 0
        relu = i < L - 1
        gdt = "f32" if i == L - 1 else xdt[i + 1]          # gy has the dtype of the consumer's input gradient
        launches = 1 if relu else 0
        names = []
        if N <= 16 and K % 4 == 0 and gdt == "f32" and not (shared and need_gx):
            spec = dict(wgrad="narrow", bias_bf16=False, gx="narrow" if need_gx else None, gx_bf16=xdt[i] == "bf16")
            names.append("k_head_bwd<%s,%s,NP=%d>" % (xdt[i], xdt[i] if need_gx else "-", 12 if N <= 12 else 16))
            launches += 2                                   # k_head_bwd + k_head_tail
            nslab = S
        else:
            ntk, ntn = -(-K // 128), -(-N // 64)
            nsplit = min(S, 8) if (ntk * ntn < 64 and S > 1) else 1
            while nsplit > 1 and (nsplit * 2 * N * K + S * N) * 4 > WS_SLAB_BYTES:      # the partial slabs must fit the workspace
                nsplit -= 1
            xcd = ntk >= 4 and ntn >= 8
            if mode == "f32":
                kern = "k_wgrad_f32"
            elif xdt[i] == "bf16" and gdt == "bf16" and K % 8 == 0 and N % 8 == 0:
                kern = "dma8?"                              # + M % 256 == 0, decided by the caller who knows M
            else:
                kern = "k_wgrad_bf16<%s,%s>" % (xdt[i] == "bf16", gdt == "bf16")
            names.append("%s nsplit=%d%s" % (kern, nsplit, " xcd_map" if xcd else ""))
            launches += 1 if nsplit == 1 else 2 + 3         # split: + k_wgrad_reduce, bnn_colsum, bnn_sample_affine_bwd, bnn_kl_backward
            how = None
            if need_gx:
                if (not shared and mode == "bf16" and xdt[i] == "bf16" and N > 16 and N % 8 == 0 and K % 8 == 0 and gdt == "bf16"):
                    how = "drawn"
                    launches += 2                           # bnn_transpose_bf16 + bnn_dense_forward
                elif K % 4 == 0 and N % (8 if gdt == "bf16" else 4) == 0:
                    how = "redraw_bf16" if mode == "bf16" else "redraw_f32"
                    launches += 1
                else:
                    how = "plain"
                    launches += 2                           # the draw + k_dgrad_plain
                if shared:
                    launches += 1                           # bnn_mc_sum over the samples
                names.append("gx " + how)
            spec = dict(wgrad=mode, bias_bf16=(mode == "bf16" and nsplit == 1), gx=how, gx_bf16=xdt[i] == "bf16")
            nslab = nsplit
        plan.append(dict(spec=spec, names=names, launches=launches, x=xdt[i], g=gdt, relu=relu, shared=shared, nslab=nslab))
    return plan


def finish_plan(plan, M):
    for p in plan:
        p["names"] = [n.replace("dma8?", "k_wgrad_bf16_dma8" if M % 256 == 0 else "k_wgrad_bf16<True,True>") for n in p["names"]]
        if p["spec"]["wgrad"] == "narrow":
            p["nslab"] *= -(-M // 256)
    return plan


# =================================================================================================== the fp32 emulation
def bf(t):
    return t.to(torch.bfloat16)


def trunc_bf16(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def epilogue32(dW, eps, mu, rho, kl, prior, nslab, mutant):
    """sum over the samples, the KL terms (kl_grad_terms) and dsoftplus, operation by operation in fp32."""
    gm = torch.zeros_like(dW[0])
    P = torch.zeros_like(dW[0])
    for s in range(dW.shape[0]):
        gm = gm + dW[s]
        P = P + dW[s] * eps[s]
    ds = torch.sigmoid(rho)
    dr = torch.zeros_like(P)
    if kl is not None:
        nb = 1.0 if mutant == "kl_without_n_batches" else kl["n_batches"]
        c = torch.tensor(kl["up"], dtype=torch.float32) * torch.tensor(1.0 / (mu.numel() * kl["T"] * nb), dtype=torch.float32)
        pm, ps = torch.tensor(prior[0], dtype=torch.float32), torch.tensor(prior[1], dtype=torch.float32)
        inv = 1.0 / (ps * ps)
        sg = 1e-10 + torch.nn.functional.softplus(rho)
        rep = float(nslab) if mutant == "kl_per_slab" else 1.0
        gm = gm + rep * (c * (mu - pm) * inv)
        dr = rep * (c * (sg * inv - 1.0 / sg))
    if mutant == "no_dsoftplus":
        return gm, P + dr
    if mutant == "dsoftplus_on_likelihood_only":
        return gm, P * ds + dr
    return gm, (P + dr) * ds


MUTANTS = ["drop_last_row", "pair_next_sample", "eps_of_sample_0", "eps_block_shift", "no_dsoftplus", "dsoftplus_on_likelihood_only",
           "kl_without_n_batches", "kl_per_slab", "relu_ge", "truncate_bf16", "swap_bias_columns", "head_gx_bf16_weights"]


def emulate(op, mutant=None):
    """What the kernels named by op["spec"] compute, in fp32 torch; mutant: one of MUTANTS, a wrong kernel."""
    spec, kl = op["spec"], op["kl"]
    x, g, y = op["x"], op["g"], op["y"]
    if y is None:
        gy = g
    else:
        keep = (y.float() >= 0) if mutant == "relu_ge" else (y.float() > 0)
        gy = torch.where(keep, g, torch.zeros_like(g))
    S, M, N = gy.shape
    rnd = (lambda t: bf(t).float()) if spec["wgrad"] == "bf16" else (lambda t: t.float())
    xs, gs = rnd(x).expand(S, -1, -1), rnd(gy)
    xw, gw = xs, gs
    if mutant == "drop_last_row":
        xw, gw = xs[:, :-1], gs[:, :-1]
    if mutant == "pair_next_sample":
        gw = gs.roll(-1, 0)
    dW = gw.transpose(1, 2) @ xw
    eps = op["eps_w"]
    K = eps.shape[2]
    if mutant == "eps_of_sample_0":
        eps = eps[:1].expand(S, -1, -1)
    if mutant == "eps_block_shift" and spec["wgrad"] != "narrow" and K % 128 != 0:
        k0 = K // 128 * 128                                # the ragged k-tile: eps of the NEXT Philox block
        flat = eps.reshape(S, -1)
        eps = eps.clone()
        eps[:, :, k0:] = flat.roll(-4, 1).reshape(S, N, K)[:, :, k0:]
    out = {}
    out["g_mu_w"], out["g_rho_w"] = epilogue32(dW, eps, op["mu_w"], op["rho_w"], kl, kl and kl["prior_w"], op["nslab"], mutant)
    if op["mu_b"] is not None:
        gb = bf(gy).float() if spec["bias_bf16"] else gy.float()
        cs = gb.sum(1)                                     # (S, N)
        if mutant == "swap_bias_columns" and N >= 32:
            cs = cs.clone()
            cs[:, 0:16], cs[:, 16:32] = cs[:, 16:32].clone(), cs[:, 0:16].clone()
        out["g_mu_b"], out["g_rho_b"] = epilogue32(cs, op["eps_b"], op["mu_b"], op["rho_b"], kl, kl and kl["prior_b"],
                                                   op["nslab"], mutant)
    how = spec["gx"]
    if how is not None:
        if how in ("narrow", "redraw_f32", "plain"):
            w = bf(op["w32"]).float() if (how == "narrow" and mutant == "head_gx_bf16_weights") else op["w32"]
            a = gy.float()
        else:
            w, a = op["wbf"].float(), bf(gy).float()
        acc = a @ w
        if spec["gx_bf16"]:
            acc = trunc_bf16(acc) if mutant == "truncate_bf16" else bf(acc)
        out["gx"] = acc
    return out


def synthetic_step(dims, B, S, mode, x_bf16, seed=0):
    """A forward and the chain of teacher-forced backward operands of a network, all in torch on the CPU: the stand-in for what
    the GPU tests capture on the device.  -> [op per layer], first layer first."""
    gen = torch.Generator().manual_seed(seed)
    plan = finish_plan(layer_plan(dims, S, mode, x_bf16), B)
    L = len(dims) - 1
    kl = dict(up=float(np.float32(KL_C)), T=2 * L, n_batches=float(N_BATCHES), prior_w=PRIOR, prior_b=PRIOR)
    x = torch.randn(B, dims[0], generator=gen)
    h = (bf(x) if x_bf16 else x).unsqueeze(0)
    ops_ = []
    for i in range(L):
        mu_w, rho_w, mu_b, rho_b = seeded.posterior(gen, (dims[i + 1], dims[i]))
        eps_w = torch.randn(S, dims[i + 1], dims[i], generator=gen)
        eps_b = torch.randn(S, dims[i + 1], generator=gen)
        w32 = mu_w + (1e-10 + torch.nn.functional.softplus(rho_w)) * eps_w
        b32 = mu_b + (1e-10 + torch.nn.functional.softplus(rho_b)) * eps_b
        wbf = bf(w32)
        p = plan[i]
        a = h.expand(S, -1, -1)
        if mode == "bf16":
            t = bf(a).float() @ wbf.float().transpose(1, 2) + b32.unsqueeze(1)
        else:
            t = a.float() @ w32.transpose(1, 2) + b32.unsqueeze(1)
        if p["relu"]:
            t = t.clamp_min(0)
            if i + 1 < L and plan[i + 1]["x"] == "bf16":
                t = bf(t)
        ops_.append(dict(spec=p["spec"], kl=kl, nslab=p["nslab"], x=h, y=t if p["relu"] else None, mu_w=mu_w, rho_w=rho_w,
                         mu_b=mu_b, rho_b=rho_b, eps_w=eps_w, eps_b=eps_b, w32=w32, wbf=wbf))
        h = t
    g = torch.randn(S, B, dims[-1], generator=gen)
    for i in reversed(range(L)):
        ops_[i]["g"] = g
        g = emulate(ops_[i]).get("gx")
    return ops_


CPU_CFG = dict(dims=(72, 40, 10), B=300, S=2, mode="bf16", x_bf16=False)        # the smallest GPU configuration ("slices")
# the same with K = 200 in the first layer: a full k-tile and a ragged one (72 columns), so that a mutant confined to the ragged
# tile leaves the full tile's 128 columns right
CPU_CFG_TWO_TILES = dict(CPU_CFG, dims=(200, 40, 10))


def _cpu_step(cfg):
    ops_ = synthetic_step(**cfg)
    return ops_, [bwdref.layer_backward(op) for op in ops_]


@pytest.fixture(scope="module")
def cpu_step():
    return _cpu_step(CPU_CFG)


@pytest.fixture(scope="module")
def cpu_step_two_tiles():
    return _cpu_step(CPU_CFG_TWO_TILES)


def test_plan_of_the_cpu_configuration():
    plan = finish_plan(layer_plan((72, 40, 10), 2, "bf16", False), 300)
    assert [p["names"] for p in plan] == [["k_wgrad_bf16<False,True> nsplit=2"], ["k_head_bwd<bf16,bf16,NP=12>"]]
    assert plan[1]["nslab"] == 4 and plan[0]["nslab"] == 2


@pytest.mark.parametrize("which", ["slices", "two_k_tiles"])
def test_emulation_is_inside_the_bound(cpu_step, cpu_step_two_tiles, which):
    """Zero violations for every output tensor of every layer; were there one, the derivation would be wrong, not the emulation."""
    ops_, refs = cpu_step if which == "slices" else cpu_step_two_tiles
    for i, (op, ref) in enumerate(zip(ops_, refs)):
        worst = bwdref.check(emulate(op), ref, "layer %d" % i)
        print("layer %d: worst |err| / bound %s" % (i, {k: round(v, 4) for k, v in worst.items()}))
        assert set(worst) == {"g_mu_w", "g_rho_w", "g_mu_b", "g_rho_b"} | ({"gx"} if i else set())


@pytest.mark.parametrize("mutant", MUTANTS)
def test_bound_rejects_the_mutant(cpu_step, mutant):
    """Each wrong kernel leaves the bound in at least one element of at least one tensor -- and the helper raises for it."""
    ops_, refs = cpu_step
    hits = []
    for i, (op, ref) in enumerate(zip(ops_, refs)):
        got = emulate(op, mutant)
        for name, (r, b, is_bf16) in ref.items():
            bad, _ = bwdref.compare(got[name], r, b, is_bf16)
            if bool(bad.any()):
                hits.append((i, name, int(bad.sum()), bad.numel()))
    print("mutant %-30s rejected at (layer, tensor, elements out, of): %s" % (mutant, hits))
    assert hits, mutant
    i = hits[0][0]
    with pytest.raises(AssertionError):
        bwdref.check(emulate(ops_[i], mutant), refs[i])


def test_bound_rejects_an_eps_shift_confined_to_the_ragged_k_tile(cpu_step_two_tiles):
    """K = 200: the mutant shifts the eps of columns 128 .. 199 by one Philox block and leaves the full tile alone.  g_rho of the
    first layer is outside the bound in the ragged tile -- and nowhere else."""
    ops_, refs = cpu_step_two_tiles
    assert ops_[0]["eps_w"].shape[2] == 200
    got = emulate(ops_[0], "eps_block_shift")
    r, b, is_bf16 = refs[0]["g_rho_w"]
    bad, _ = bwdref.compare(got["g_rho_w"], r, b, is_bf16)
    print("ragged-tile eps shift: %d of %d elements of the ragged tile out, %d of the full tile" % (int(bad[:, 128:].sum()), bad[:, 128:].numel(), int(bad[:, :128].sum())))
    assert int(bad[:, :128].sum()) == 0 and int(bad[:, 128:].sum()) > 0.9 * bad[:, 128:].numel()
    for name in ("g_mu_w", "g_mu_b", "g_rho_b"):
        assert not bool(bwdref.compare(got[name], *refs[0][name])[0].any())
    with pytest.raises(AssertionError):
        bwdref.check(got, refs[0])


# =================================================================================================== host: argument checks
BAD_KEY = dict(seed=1, stream=70000)                      # a stream id beyond 65535: check_rng refuses it
UNLAUNCHABLE_M = 256 * 65536 + 1                           # 65537 row slices: beyond gridDim.z, refused at the workspace check


def narrow_call(lib, ldgx, rng_w, rng_b, M):
    """bnn_linear_backward_narrow_sampled on pointers that are never dereferenced on the host.  Every call of these tests carries,
    besides the argument under test, a SECOND reason for refusal that the host meets later and still before its first launch --
    so a library without the check under test fails the assertion and launches nothing either, workspace registered or not."""
    one = ctypes.c_void_p(64)
    K, N, S = 40, 10, 2
    return lib.bnn_linear_backward_narrow_sampled(one, M * K, K, one, M * N, N, one, one, one, M * ldgx, ldgx, one, one, one, one, one,
                                                  M, N, K, S, ctypes.byref(rng_w), ctypes.byref(rng_b), None, 0, 0, None)


def test_narrow_backward_refuses_a_misaligned_gx_pitch_without_launching():
    """gx rows are stored as float4 / uint2 at gx + s stride + m ldgx + k: a pitch of K + 1 passes the extent check and must not
    pass the alignment gate (callers fall back to the general kernels on E_ALIGN).  Second refusal: a bad weight key, which is
    checked right after the gate."""
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    bad, good = _lib.Rng(**BAD_KEY), _lib.Rng(seed=1, stream=8)
    bad_key = lib.bnn_eps_philox(ctypes.c_void_p(64), 4, 1, 4, ctypes.byref(bad), None)
    assert bad_key < 0 and bad_key != _lib.E_ALIGN
    assert narrow_call(lib, 41, bad, good, 8) == _lib.E_ALIGN
    assert b"misaligned" in lib.bnn_last_error()
    assert narrow_call(lib, 40, bad, good, 8) == bad_key     # the same call with a legal pitch gets as far as the key
    assert lib.bnn_launch_count() == n0


def test_narrow_backward_checks_the_bias_key_before_launching():
    """A bad bias key is refused with the key's own code, with the other argument checks.  Second refusal: 65537 row slices,
    which the workspace check -- the last one before the launch -- turns down as E_UNSUPPORTED whatever workspace is registered."""
    lib = _lib.load()
    n0 = lib.bnn_launch_count()
    bad, good = _lib.Rng(**BAD_KEY), _lib.Rng(seed=1, stream=8)
    bad_key = lib.bnn_eps_philox(ctypes.c_void_p(64), 4, 1, 4, ctypes.byref(bad), None)
    assert bad_key < 0 and bad_key != _lib.E_UNSUPPORTED
    assert narrow_call(lib, 40, good, bad, UNLAUNCHABLE_M) == bad_key
    assert b"rng_b" in lib.bnn_last_error()
    assert narrow_call(lib, 40, good, good, UNLAUNCHABLE_M) == _lib.E_UNSUPPORTED     # good keys: only the second refusal is left
    assert lib.bnn_launch_count() == n0


# =================================================================================================== GPU
GPU_CFGS = {
    # L1 dma8: 4 x 9 tiles < 64 -> the sample split, xcd_map on, shared x (x_sample_stride 0); three slabs of 2 x 520 x 392 floats
    #   do not fit the 4 MiB workspace, so the host settles on nsplit = 2 for the 3 samples: an UNEVEN split (samples 0 | 1, 2).
    #   The shape is kept as specified: the branch it was chosen for (dma8 + sample split + xcd_map + shared x) is the one that runs,
    #   ntn >= 8 with fewer than 64 tiles needs N >= 456 at K >= 385, and an uneven split is the harder case of the two;
    #   bias via bnn_colsum, bnn_sample_affine_bwd, bnn_kl_backward
    # L2 dma8: 5 x 5 tiles, split three ways, plain tile order; input gradient on the drawn weights
    # head: narrow <bf16 x, bf16 gx, NP = 12>, ragged last 64-column block (264 = 4 * 64 + 8), fused KL
    "split": dict(dims=(392, 520, 264, 10), B=256, S=3, mode="bf16", x_bf16=True, names=[
        ["k_wgrad_bf16_dma8 nsplit=2 xcd_map"], ["k_wgrad_bf16_dma8 nsplit=3", "gx drawn"], ["k_head_bwd<bf16,bf16,NP=12>"]]),
    # L1 dma8 in one pass: 7 x 10 = 70 tiles, xcd_map with odd ntk and ntn % 4 != 0 (masked workgroups), bias + KL fused in the store
    # L2 split two ways
    "onepass": dict(dims=(784, 584, 72, 10), B=256, S=2, mode="bf16", x_bf16=True, names=[
        ["k_wgrad_bf16_dma8 nsplit=1 xcd_map"], ["k_wgrad_bf16_dma8 nsplit=2", "gx drawn"], ["k_head_bwd<bf16,bf16,NP=12>"]]),
    # L1 <fp32 x, bf16 gy>; L2 <bf16, bf16> register-staged (M % 256 != 0); L3 N = 24 > 16 with fp32 gy: <bf16 x, fp32 gy>, input
    # gradient through the fused re-draw kernel with fp32 gy and bf16 gx.  S = 3: everything split
    "ragged3": dict(dims=(200, 136, 72, 24), B=72, S=3, mode="bf16", x_bf16=False, names=[
        ["k_wgrad_bf16<False,True> nsplit=3"], ["k_wgrad_bf16<True,True> nsplit=3", "gx drawn"],
        ["k_wgrad_bf16<True,False> nsplit=3", "gx redraw_bf16"]]),
    # S = 1: nothing split; bias and KL fused in the register-staged kernel at ragged N; every input shared (fp32 gx partial, rounded after)
    "ragged1": dict(dims=(200, 136, 72, 24), B=72, S=1, mode="bf16", x_bf16=False, names=[
        ["k_wgrad_bf16<False,True> nsplit=1"], ["k_wgrad_bf16<True,True> nsplit=1", "gx redraw_bf16"],
        ["k_wgrad_bf16<True,False> nsplit=1", "gx redraw_bf16"]]),
    # narrow kernel with two row slices (M > 256); L1 <fp32 x, bf16 gy> with K % 128 != 0 and N % 64 != 0
    "slices": dict(dims=(72, 40, 10), B=300, S=2, mode="bf16", x_bf16=False, names=[
        ["k_wgrad_bf16<False,True> nsplit=2"], ["k_head_bwd<bf16,bf16,NP=12>"]]),
    # fp32 parity: k_wgrad_f32 split, the fp32 narrow kernel with KL and bias, the fp32 fused input gradient
    "parity_split": dict(dims=(392, 520, 264, 10), B=64, S=3, mode="f32", x_bf16=False, names=[
        ["k_wgrad_f32 nsplit=2 xcd_map"], ["k_wgrad_f32 nsplit=3", "gx redraw_f32"], ["k_head_bwd<f32,f32,NP=12>"]]),
    "parity_slices": dict(dims=(72, 40, 10), B=300, S=2, mode="f32", x_bf16=False, names=[
        ["k_wgrad_f32 nsplit=2"], ["k_head_bwd<f32,f32,NP=12>"]]),
    # S = 1: k_wgrad_f32 unsplit with bias and KL fused; the head's shared input keeps it off the narrow kernel (plain input gradient)
    "parity_one": dict(dims=(72, 40, 10), B=300, S=1, mode="f32", x_bf16=False, names=[
        ["k_wgrad_f32 nsplit=1"], ["k_wgrad_f32 nsplit=1", "gx plain"]]),
}


def device_step(cfg, seed, prepare=None, kl_c=KL_C):
    """One forward + backward on the device with every layer's operands captured -> ([op per layer], [got per layer], launches of
    the backward).  prepare(net): applied to the network on the device before the step (tests/test_posterior_range.py prunes it);
    kl_c: the KL term's weight in the loss (0: the likelihood's gradient alone)."""
    import bayesianneuralnetworks_amd as bnn
    from bayesianneuralnetworks_amd import ops
    from bayesianneuralnetworks_amd.nn import NormalLinear, KLDivergence, BayesianNetworkModule, fuse_activations, fuse_kl_gradient
    from bayesianneuralnetworks_amd._rng import default_generator
    dev = torch.device("cuda:0")
    dims, B, S, mode = cfg["dims"], cfg["B"], cfg["S"], cfg["mode"]
    L = len(dims) - 1
    plan = finish_plan(layer_plan(dims, S, mode, cfg["x_bf16"]), B)
    # the host's dispatch conditions, restated in layer_plan, send these shapes to the branches they were chosen for.  (The kernel
    # names are DERIVED, not observed: what the device confirms below is the backward's launch count -- which tells narrow, split,
    # unsplit, drawn, re-drawn and plain apart -- and every layer's operand dtypes and shared flag.)
    assert [p["names"] for p in plan] == cfg["names"]

    class Net(BayesianNetworkModule):
        def __init__(self):
            super().__init__(dims[0], dims[-1], samples=S)
            mods = []
            for i in range(L):
                mods.append(NormalLinear(dims[i], dims[i + 1]))
                if i < L - 1:
                    mods.append(torch.nn.ReLU())
            self.layers = torch.nn.Sequential(*mods)

        def _forward(self, x):
            return self.layers(x)

    # process-wide state this step touches, put back at the end: the eps generator's seed and draw counter, the device epoch
    # words, the KL-fusion switch
    saved_gen = (default_generator._seed, default_generator._torch_seed, default_generator.epoch_host)
    saved_cells = [(cell, cell.clone()) for cell in default_generator._epoch_dev.values()]
    saved_fuse = ops.FUSE_KL_GRADIENT
    for cell in default_generator._epoch_dev.values():
        cell.zero_()
    net = Net()
    pgen = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():                                   # the posterior from the test's own generator, not torch's global one
        for m in net.layers:
            if isinstance(m, NormalLinear):
                for p_, v in zip((m.weight.mean, m.weight.scale, m.bias.mean, m.bias.scale), seeded.posterior(pgen, tuple(m.weight.mean.shape))):
                    p_.copy_(v)
    net = net.to(dev)
    seeded.pin_streams(net, 4000 + 16 * seed)
    net.mc_batched = True
    if prepare is not None:
        prepare(net)
    layers = [m for m in net.layers if isinstance(m, NormalLinear)]
    for m in layers:
        m.compute = mode
    fuse_activations(net, bf16_activations=(mode == "bf16"))
    bnn.manual_seed(77 + seed)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, dims[0], generator=gen).to(dev)
    if cfg["x_bf16"]:
        x = x.to(torch.bfloat16)
    gy0 = torch.randn(S, B, dims[-1], generator=gen).to(dev)
    cap = [dict() for _ in layers]
    handles = []
    for i, m in enumerate(layers):
        def hook(mod, inp, out, i=i):
            cap[i]["x"], cap[i]["y"] = inp[0].detach(), out.detach()
            out.register_hook(lambda g, i=i: cap[i].__setitem__("g", g.detach().clone()))
        handles.append(m.register_forward_hook(hook))
    lib = _lib.load()
    fuse_kl_gradient(True)
    try:
        ys = net.forward_stacked(x, S)
        loss = (ys * gy0).sum() + kl_c * KLDivergence(number_of_batches=N_BATCHES)(net)
        n0 = lib.bnn_launch_count()
        loss.backward()
        torch.cuda.synchronize()
        launches = lib.bnn_launch_count() - n0
    finally:
        fuse_kl_gradient(saved_fuse)
        for h in handles:
            h.remove()
    try:
        return _collect(cfg, plan, layers, cap, launches, dev, kl_c)
    finally:                                                # (the draws above are re-created from the keys before the state goes back)
        default_generator._seed, default_generator._torch_seed, default_generator.epoch_host = saved_gen
        for cell, was in saved_cells:
            cell.copy_(was)


def _collect(cfg, plan, layers, cap, launches, dev, kl_c=KL_C):
    """The captured operands and the gradients of device_step's backward, on the CPU."""
    from bayesianneuralnetworks_amd import ops
    dims, B, S = cfg["dims"], cfg["B"], cfg["S"]
    L = len(dims) - 1
    assert not ops._tls.kl_pending, "a parked KL gradient was left behind"
    _lib.check_device(dev)
    kl = dict(up=float(np.float32(kl_c)), T=2 * L, n_batches=float(N_BATCHES), prior_w=PRIOR, prior_b=PRIOR)
    ops_, gots = [], []
    for i, (m, p) in enumerate(zip(layers, plan)):
        K, N = dims[i], dims[i + 1]
        for prior in (m.weight_prior, m.bias_prior):        # (Normal's parameters are fp32 tensors; kl_grad64 rounds PRIOR the same way)
            assert (float(prior.loc), float(prior.scale)) == tuple(float(np.float32(v)) for v in PRIOR)
        kw, kb = m.weight.draw_key, m.bias.draw_key
        assert kw.nsamples == S and kb.nsamples == S
        mu_w, rho_w, mu_b, rho_b = (t.detach() for t in (m.weight.mean, m.weight.scale, m.bias.mean, m.bias.scale))
        xi = cap[i]["x"]
        assert str(xi.dtype).endswith("bfloat16" if p["x"] == "bf16" else "float32"), (i, xi.dtype)
        assert str(cap[i]["g"].dtype).endswith("bfloat16" if p["g"] == "bf16" else "float32"), (i, cap[i]["g"].dtype)
        assert (xi.shape[0] == B) == p["shared"]
        op = dict(spec=p["spec"], kl=kl, nslab=p["nslab"], x=xi.reshape(-1, B, K), g=cap[i]["g"].reshape(S, B, N),
                  y=cap[i]["y"].reshape(S, B, N) if p["relu"] else None, mu_w=mu_w, rho_w=rho_w, mu_b=mu_b, rho_b=rho_b,
                  eps_w=ops.eps_philox((N, K), kw, dev), eps_b=ops.eps_philox((N,), kb, dev))
        if p["spec"]["gx"] is not None:
            op["w32"] = ops._sample_affine_philox_raw(mu_w, rho_w, kw)
            op["wbf"] = ops._sample_affine_philox_raw(mu_w, rho_w, kw, torch.bfloat16)
        ops_.append({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in op.items()})
        got = dict(g_mu_w=m.weight.mean.grad, g_rho_w=m.weight.scale.grad, g_mu_b=m.bias.mean.grad, g_rho_b=m.bias.scale.grad)
        if i > 0:
            got["gx"] = cap[i - 1]["g"].reshape(S, B, K)
        gots.append({k: v.detach().cpu() for k, v in got.items()})
    return ops_, gots, launches, plan


@gpu
@pytest.mark.parametrize("name", list(GPU_CFGS))
def test_backward_of_every_layer_against_float64(name):
    cfg = GPU_CFGS[name]
    ops_, gots, launches, plan = device_step(cfg, seed=1 + list(GPU_CFGS).index(name))
    want = sum(p["launches"] for p in plan)
    print("%s: backward launches %d (the plan's kernels: %d) %s" % (name, launches, want, [p["names"] for p in plan]))
    out_dir = os.environ.get(RECORD_DIR_ENV, "")             # where a run keeps its measured figures, if it keeps any
    fails = []
    for i, (op, got) in enumerate(zip(ops_, gots)):
        ref = bwdref.layer_backward(op)
        assert set(ref) == set(got), (i, set(ref) ^ set(got))
        try:
            worst = bwdref.check(got, ref, "%s layer %d (%s)" % (name, i, ", ".join(plan[i]["names"])))
        except AssertionError as e:
            fails.append(str(e))
            worst = {k: float(bwdref.compare(got[k], *ref[k])[1].max()) for k in ref}
        print("%s layer %d %s: worst |err| / bound %s" % (name, i, plan[i]["names"], {k: round(v, 4) for k, v in worst.items()}))
        if os.path.isdir(out_dir):                           # measured ratios next to the bound, for the record
            with open(os.path.join(out_dir, "train_step_check.jsonl"), "a") as f:
                for k, v in worst.items():
                    f.write(json.dumps(dict(config=name, layer=i, tensor=k, kernels=plan[i]["names"], worst_ratio=v)) + "\n")
    assert not fails, "\n".join(fails)
    assert launches == want, (launches, want)
