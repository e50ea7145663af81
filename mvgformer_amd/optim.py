"""The optimizer step of the training loop on the device: torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam / AdamW
(lib/core/function.py:167-178, run/train_3d.py:116-146) and the reference's `if losses > 0` guard, as ONE call of the fused HIP
kernels of csrc/optim.hip: at most three launches whatever the number of parameter tensors is, fixed-order fp64 sums, nothing read
back by the host, so the step can be captured in a HIP graph.

  FusedAdam   a torch.optim.Optimizer: param_groups, lr schedulers, state_dict() / load_state_dict() as torch.optim.Adam's

There is no fall-back to torch: amsgrad, maximize, tensor hyper-parameters, sparse gradients and parameters that are not
contiguous fp32 raise."""
from __future__ import annotations

import torch

from . import ops

CHUNK = ops.OPTIM_CHUNK           # elements of one tensor that one workgroup handles (MVG_OPTIM_CHUNK)

_TORCH_ADAM_KEYS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)


def _check_param(p):
    if not isinstance(p, torch.Tensor):
        raise TypeError("FusedAdam: parameters must be tensors, got %s" % type(p).__name__)
    if p.dtype != torch.float32:
        raise TypeError("FusedAdam: float32 parameters only, got %s (the kernels keep fp32 master weights)" % p.dtype)
    if p.layout != torch.strided or not p.is_contiguous():
        raise ValueError("FusedAdam: parameters must be dense and contiguous")


class FusedAdam(torch.optim.Optimizer):
    """Adam (weight decay added to the gradient) or AdamW (decoupled_weight_decay=True) with the gradient-norm clip of
    clip_grad_norm_(parameters, clip_max_norm) in front, over all parameters of all groups at once.

    step(loss=None) returns the total gradient norm before clipping as a device fp32 scalar (what clip_grad_norm_ returns).  With
    `loss` (the step's total as a device scalar) the step is skipped on the device unless loss > 0, the reference's guard: no
    parameter, moment or step count changes; a NaN loss skips too.  After the step the gradients hold the clipped values, or
    zeros with zero_grad=True (in place, never None: the tables below stay valid from the second step on).

    The kernels are driven by tables in device memory (one record per tensor / per 4096-element chunk / per group).  They are
    rebuilt and uploaded only when the set of (parameter, gradient) pointers changes; the group hyper-parameters are compared
    with the last upload on the host and re-sent with one pinned, non-blocking copy when they differ (a scheduler step).
    prepare() does both ahead of a HIP-graph capture; step() inside a capture with stale tables raises.

    One step count serves all parameters (it lives on the device); state_dict() reads it back and writes it into every
    parameter's state, so the layout is torch.optim.Adam's (step, exp_avg, exp_avg_sq) and state dicts move both ways.  A
    parameter whose first gradient arrives later starts with zero moments and shares that count.

    Every updated parameter's version counter is bumped after the launch (torch.autograd.graph.increment_version): the kernels
    write through raw pointers, and the decoder's operand caches (projattn.WeightCache) are keyed on the version.  A graph
    replay does not run this host code: call mark_updated() after replays, before the next forward."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled_weight_decay=False,
                 clip_max_norm=0.0, zero_grad=False, amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise NotImplementedError("FusedAdam: amsgrad / maximize are not built")
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise NotImplementedError("FusedAdam: lr / betas as tensors are not built (python floats; schedulers write floats)")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid beta parameters: %r" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        self.clip_max_norm, self.zero_grad_after_step = float(clip_max_norm), bool(zero_grad)
        self._state_dev = None        # int64 state block (ops.optim_state_words); word 0 = the step count
        self._step_host = 0           # the count while there is no state block yet (before the first step / after a load)
        self._tables = None           # (signature, tensor_table, chunk_table, workspace, updated parameters)
        self._groups_dev, self._groups_host = None, None
        self._operands = None         # attach_operands
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                        decoupled_weight_decay=bool(decoupled_weight_decay), **_TORCH_ADAM_KEYS)
        super().__init__(params, defaults)

    # ---- torch.optim.Optimizer surface -----------------------------------------------------------------------------------------
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            _check_param(p)
        if len(self.param_groups) > 64:
            raise ValueError("FusedAdam: at most 64 parameter groups")
        self._groups_host = None

    def __setstate__(self, state):
        super().__setstate__(state)
        for k, v in (("_state_dev", None), ("_step_host", 0), ("_tables", None), ("_groups_dev", None), ("_groups_host", None),
                     ("_operands", None), ("clip_max_norm", 0.0), ("zero_grad_after_step", False)):
            self.__dict__.setdefault(k, v)
        for group in self.param_groups:
            for k, v in _TORCH_ADAM_KEYS.items():
                group.setdefault(k, v)
            group.setdefault("decoupled_weight_decay", self.defaults["decoupled_weight_decay"])
            if group["amsgrad"] or group["maximize"]:
                raise NotImplementedError("FusedAdam: amsgrad / maximize are not built")

    def state_dict(self):
        """torch.optim.Adam's layout.  Reads the device step count (one synchronisation)."""
        sd = super().state_dict()
        step = float(self.step_count())
        sd["state"] = {k: {"step": torch.tensor(step, dtype=torch.float32), **{n: v for n, v in st.items() if n != "step"}}
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        steps = {float(st["step"]) for st in state_dict["state"].values() if "step" in st}
        if len(steps) > 1:
            raise ValueError("FusedAdam keeps one step count for all parameters; the state to load has %s" % sorted(steps))
        super().load_state_dict(state_dict)
        for p, st in self.state.items():
            st.pop("step", None)
            for k in ("exp_avg", "exp_avg_sq"):       # own memory: load_state_dict may hand out the saved tensors themselves
                if k in st:
                    st[k] = st[k].detach().to(torch.float32).clone(memory_format=torch.contiguous_format)
        self._set_step(int(steps.pop()) if steps else 0)
        self._tables, self._groups_host = None, None

    def zero_grad(self, set_to_none=False):
        """in place by default: a gradient set to None is re-allocated by the next backward and forces a table upload"""
        super().zero_grad(set_to_none=set_to_none)

    # ---- step count ------------------------------------------------------------------------------------------------------------
    def step_count(self):
        """optimizer steps taken (skipped ones not counted); synchronises if a step has run"""
        if self._state_dev is None:
            return self._step_host
        return int(self._state_dev[0].item())

    def last_total_norm(self):
        """the last step's gradient norm before clipping as the kernels summed it: an fp64 device scalar (a view of the state
        block, overwritten by the next step; no synchronisation)"""
        if self._state_dev is None:
            raise RuntimeError("FusedAdam.last_total_norm: no step has run")
        return self._state_dev.view(torch.float64)[1]

    def _set_step(self, n):
        self._step_host = int(n)
        if self._state_dev is not None:
            self._state_dev[0:1].fill_(int(n))

    # ---- device tables ---------------------------------------------------------------------------------------------------------
    def _device(self):
        dev = None
        for group in self.param_groups:
            for p in group["params"]:
                if not p.is_cuda:
                    raise RuntimeError("Not implemented on the CPU")      # the package's message (ops / _lib.require_cuda)
                if dev is None:
                    dev = p.device
                elif p.device != dev:
                    raise RuntimeError("FusedAdam: parameters on %s and %s; one optimizer per device" % (dev, p.device))
        if dev is None:
            raise RuntimeError("FusedAdam: no parameters")
        return dev

    def _signature(self):
        """what the tensor table depends on: (p, grad) pointers, sizes and group of every parameter with a gradient"""
        sig, params = [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                sig.append((p.data_ptr(), g.data_ptr(), p.numel(), gi))
                params.append(p)
        return tuple(sig), params

    def _group_rows(self):
        rows = []
        for group in self.param_groups:
            lr, (b1, b2) = group["lr"], group["betas"]
            if any(isinstance(x, torch.Tensor) for x in (lr, b1, b2, group["eps"], group["weight_decay"])):
                raise NotImplementedError("FusedAdam: hyper-parameters as tensors are not built")
            if group["amsgrad"] or group["maximize"]:
                raise NotImplementedError("FusedAdam: amsgrad / maximize are not built")
            rows.append((float(lr), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                         1.0 if group["decoupled_weight_decay"] else 0.0))
        return rows

    @staticmethod
    def _capturing():
        return torch.cuda.is_current_stream_capturing()

    def _sync_groups(self, dev):
        rows = self._group_rows()
        if rows == self._groups_host and self._groups_dev is not None:
            return
        if self._capturing():
            raise RuntimeError("FusedAdam: the group hyper-parameters on the device are stale and a HIP-graph capture is in "
                               "progress; call prepare() before capturing")
        if self._groups_dev is None or self._groups_dev.shape[0] != len(rows):
            self._groups_dev = torch.empty((len(rows), ops.OPTIM_GROUP_WORDS), dtype=torch.float64, device=dev)
        self._groups_dev.copy_(torch.tensor(rows, dtype=torch.float64).pin_memory(), non_blocking=True)
        self._groups_host = rows
        words = ops.optim_state_words(len(rows))
        if self._state_dev is None or self._state_dev.numel() < words:
            old = self._state_dev
            self._state_dev = torch.zeros((words,), dtype=torch.int64, device=dev)
            if old is not None:
                self._state_dev[0:1].copy_(old[0:1])
            elif self._step_host:
                self._state_dev[0:1].fill_(self._step_host)

    def _sync_tables(self, dev):
        sig, params = self._signature()
        if self._tables is not None and self._tables[0] == sig:
            return self._tables
        if self._capturing():
            raise RuntimeError("FusedAdam: the tensor tables are not built for the current (parameter, gradient) pointers and a "
                               "HIP-graph capture is in progress; call prepare() (with the gradients in place) before capturing")
        rows, chunks = [], []
        for ti, p in enumerate(params):
            g = p.grad
            _check_param(p)
            if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
                raise RuntimeError("FusedAdam: gradients must be dense contiguous float32 tensors of the parameter's shape")
            st = self.state[p]
            if "exp_avg" not in st:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            if any(t.dtype != torch.float32 or not t.is_contiguous() or t.shape != p.shape or t.device != p.device for t in (m, v)):
                raise RuntimeError("FusedAdam: exp_avg / exp_avg_sq must be contiguous float32 tensors of the parameter's shape")
            n = p.numel()
            rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, sig[ti][3]))
            chunks.extend((ti, c) for c in range((n + CHUNK - 1) // CHUNK))
        nt, nc = len(rows), len(chunks)
        host = torch.empty((nt * ops.OPTIM_TENSOR_WORDS + nc,), dtype=torch.int64)
        if nt:
            host[:nt * ops.OPTIM_TENSOR_WORDS] = torch.tensor(rows, dtype=torch.int64).flatten()
        if nc:
            host[nt * ops.OPTIM_TENSOR_WORDS:].view(torch.int32).copy_(torch.tensor(chunks, dtype=torch.int32).flatten())
        buf = torch.empty((max(host.numel(), 1),), dtype=torch.int64, device=dev)
        if host.numel():
            buf[:host.numel()].copy_(host.pin_memory(), non_blocking=True)
        tensor_table = buf[:nt * ops.OPTIM_TENSOR_WORDS].view(nt, ops.OPTIM_TENSOR_WORDS)
        chunk_table = buf[nt * ops.OPTIM_TENSOR_WORDS:nt * ops.OPTIM_TENSOR_WORDS + nc].view(torch.int32).view(nc, 2)
        workspace = torch.empty((max(nc, 1),), dtype=torch.float64, device=dev)
        self._tables = (sig, tensor_table, chunk_table, workspace, params)
        return self._tables

    def prepare(self):
        """Build and upload the tensor / chunk tables for the gradients as they are now and the group table for param_groups as
        they are now.  Ahead of a HIP-graph capture, and between replays after a change of param_groups (a scheduler step): the
        tables keep their addresses, so a captured step reads the new values without recapture."""
        dev = self._device()
        with torch.cuda.device(dev):
            self._sync_groups(dev)
            self._sync_tables(dev)
        return self

    def attach_operands(self, operands):
        """operands: a training.TrainOperands (or None to detach) -- the bf16 copies of the weights that the bf16 training path
        multiplies by, kept on the device.  step() then launches their refresh right behind the update kernel (one more launch,
        also inside a captured graph) and re-stamps them after its version bump, so the next forward neither re-casts the
        weights on the host's order nor reads last step's copies."""
        self._operands = operands
        return self

    @property
    def operands(self):
        """the attached training.TrainOperands, or None"""
        return self._operands

    def mark_updated(self):
        """bump the version counters of the parameters the tables cover (after graph replays: a replay runs no host code); attached
        operands were refreshed by the replayed step and are re-stamped for the new versions"""
        if self._tables is not None and self._tables[4]:
            torch.autograd.graph.increment_version(self._tables[4])
        if self._operands is not None:
            self._operands.restamp()

    @torch.no_grad()
    def step(self, loss=None, closure=None):
        if closure is not None:
            raise NotImplementedError("FusedAdam.step: closures are not supported (pass the step's loss as `loss`)")
        dev = self._device()
        if loss is not None:
            if not isinstance(loss, torch.Tensor) or loss.numel() != 1:
                raise TypeError("FusedAdam.step: loss must be a one-element tensor on the parameters' device")
            if not loss.is_cuda:
                raise RuntimeError("Not implemented on the CPU")
            loss = loss.detach()
            if loss.dtype != torch.float32:
                loss = loss.float()
        with torch.cuda.device(dev):
            self._sync_groups(dev)
            _, tensor_table, chunk_table, workspace, params = self._sync_tables(dev)
            norm = torch.empty((), dtype=torch.float32, device=dev)
            ops.optim_step(tensor_table, chunk_table, self._groups_dev, self._state_dev, workspace, loss=loss,
                           max_norm=self.clip_max_norm, zero_grad=self.zero_grad_after_step, norm_out=norm)
            if self._operands is not None:
                self._operands.launch()     # unconditionally too: the refresh is idempotent, a skipped step rewrites the same bits
        # unconditionally: the host cannot know whether the device skipped the step
        if params:
            torch.autograd.graph.increment_version(params)
        if self._operands is not None:
            self._operands.restamp()
        return norm
