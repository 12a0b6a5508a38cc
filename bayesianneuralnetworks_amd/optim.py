"""Optimizer step of the reference's training loop on the device (examples/MNIST/train.py:41,65):
torch.optim.Adam semantics (amsgrad = False, maximize = False, L2 weight_decay), every parameter
tensor of the model updated by ONE HIP launch (csrc/bnn_train.hip) -- graph-capturable, the step
counter lives on the device.

Deviations from torch.optim.Adam (pinned by tests/test_hip_parity.py::test_fused_adam_matches_torch_adam at
rtol 1e-5 against torch, and held to float64 in tests/test_train_tail.py): ONE step counter per parameter group
(torch: one per parameter -- the same value whenever every parameter of the group has a gradient, as in the
reference's loop), and hyper-parameters and bias corrections in fp32 (torch: Python doubles).  Two effects, both
relative to the update:
  * lr, betas, eps and weight_decay are passed to the device as floats.  1 - beta then carries the beta's rounding
    amplified by beta / (1 - beta): at most 2^-24 (2 + 2 b1 / (1 - b1) + b2 / (1 - b2)) = 6e-5 for the default
    betas.  Measured from arbitrary (m, v) states: 6.7e-6 for (0.9, 0.999), 7e-7 for (0.9, 0.99), about constant
    over the first 1 / (1 - b2) steps and below 1e-6 after them; 8.3e-5 for b2 = 0.9999, NOT largest at the first
    steps.  From a zero state the first steps deviate least (5e-8: the factor 1 - b2 of v and of 1 - b2^t cancels).
  * 1 - powf(beta, t) in fp32 is within 4 * 2^-24 * beta^t / (1 - beta^t) relative (halved for b2 by the square
    root): largest on the first updates -- at most 6e-5 at t = 2 for b2 = 0.999 (t = 1 is exact) -- and gone once
    beta^t is small.
The state_dict holds `step` in the group, not per parameter: it is not interchangeable with torch.optim.Adam's."""
import ctypes

import torch

from . import _lib
from ._lib import AdamTensor, BnnHipError, check, ptr, stream_ptr


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def ensure_state(self):
        """Create the moments of every parameter that requires a gradient, and every group's step counter, now -- what the first
        step() would do.  For a step that is to be CAPTURED before any eager step has run: tensors created inside a capture live
        in the graph, and the fill that zeroes them is replayed with it (step() refuses to create them there)."""
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.requires_grad]
            for p in ps:
                if not self.state[p]:
                    self._new_state(p)
            if ps and "step" not in group:
                group["step"] = torch.zeros(1, dtype=torch.float32, device=ps[0].device)

    def _new_state(self, p):
        st = self.state[p]
        st["exp_avg"] = torch.zeros_like(p)
        st["exp_avg_sq"] = torch.zeros_like(p)
        return st

    @staticmethod
    def _refuse_state_in_capture():
        if torch.cuda.is_current_stream_capturing():
            raise BnnHipError("optim.Adam: this step would create its moments or its step counter inside a graph capture, where every "
                              "replay zeroes them again; run one eager step first, or call ensure_state() before the capture")

    @torch.no_grad()
    def step(self, closure=None, advance=None):
        """advance (optional, a device epoch cell of _rng.EpsGenerator.epoch_dev): bumped by one in the step's last launch
        -- the fresh-noise step of a captured training step without a launch of its own (last parameter group only).
        The launch writes the parameters, the moments and the step counter through raw pointers; their autograd version counters
        are advanced here (host-only, nothing is added to a capture), so that whatever keys on a parameter's version -- autograd's
        check of saved tensors, the layers' operand caches -- sees the step."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        groups = [g for g in self.param_groups if any(p.grad is not None for p in g["params"])]
        if advance is not None and not groups:
            check(lib.bnn_rng_advance(ptr(advance), 1, stream_ptr(advance.device)), "bnn_rng_advance")
        for gi, group in enumerate(groups):
            ps = [p for p in group["params"] if p.grad is not None]
            dev = ps[0].device
            arr = (AdamTensor * len(ps))()
            for i, p in enumerate(ps):
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                    raise BnnHipError("optim.Adam: parameters must be contiguous fp32 tensors on one GPU")
                g = p.grad
                if g.dtype != torch.float32 or not g.is_contiguous():
                    raise BnnHipError("optim.Adam: gradients must be contiguous fp32")
                st = self.state[p]
                if not st:
                    self._refuse_state_in_capture()
                    st = self._new_state(p)
                arr[i].p, arr[i].g = p.data_ptr(), g.data_ptr()
                arr[i].m, arr[i].v, arr[i].n = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
            if "step" not in group:
                self._refuse_state_in_capture()
                group["step"] = torch.zeros(1, dtype=torch.float32, device=dev)
            adv = advance if (advance is not None and gi == len(groups) - 1) else None
            check(lib.bnn_adam_step_advance(arr, len(ps), float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]),
                                            float(group["eps"]), float(group["weight_decay"]), ptr(group["step"]),
                                            ptr(adv) if adv is not None else None, 1, stream_ptr(dev)), "bnn_adam_step")
            written = list(ps)
            for p in ps:
                written += (self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"])
            torch.autograd.graph.increment_version(written + [group["step"]])
        return loss
