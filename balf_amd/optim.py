"""``FusedAdam`` and ``FusedSGD``: ``torch.optim.Optimizer`` subclasses whose ``step()`` is ONE launch per parameter group
(``ops.adam_step`` / ``ops.sgd_step``: balf_adam_step / balf_sgd_step of include/balf_hip.h) instead of torch's
multi-launch foreach composition.  They are what ``utils.train_utils.build_optimizer`` returns for float32 parameters on the GPU and
what ``utils.train_utils.train_head`` is meant to be driven with.

Being subclasses, ``param_groups``, ``zero_grad``, ``add_param_group``, torch's lr schedulers and ``state_dict`` /
``load_state_dict`` are torch's own.  The per-parameter state uses torch's keys -- ``step`` (a CPU float32 scalar tensor, as torch
writes it), ``exp_avg``, ``exp_avg_sq`` -- so a ``state_dict()`` loads into ``torch.optim.Adam`` and one written by
``torch.optim.Adam`` (the ``optimizer_state`` of the reference's checkpoints) loads here.  Nothing in ``step()`` reads the device or
synchronises.

The kernel takes a few microseconds; what a step costs is the host's walk over the parameters.  So each group keeps
a plan: its parameters' state dictionaries, the pointers gathered by ``ops.optim_pointers`` (gathered again when a ``data_ptr`` of
a parameter or a moment has changed), and -- FusedAdam -- one CPU tensor whose elements ARE the ``step`` scalars of the group (each
``state[p]['step']`` is a 0-d view of it), so that reading every step count is one ``tolist()`` and advancing them one ``add_``.
When a plan is dropped is listed at ``_FusedOptimizer._plan``.

``step()`` cannot be captured into a graph: the step number, ``lr``, ``lr / bc1`` and ``sqrt(bc2)`` are launch arguments, passed by
value, so a replay would repeat the captured step's bias corrections and learning rate.  Under a capture it raises RuntimeError
before anything is launched (as ``torch.optim.Adam(capturable=False)`` does)."""
from __future__ import annotations

import operator

import torch

from . import _lib, ops

_RUN = _lib.OPTIM_MAX_TENSORS
_data_ptr = torch.Tensor.data_ptr
_is = operator.is_
_cuda_ready = torch.cuda.is_initialized                                  # (False on a host without a GPU: nothing is asked of one)
_capturing = getattr(torch._C, "_cuda_isCurrentStreamCapturing", torch.cuda.is_current_stream_capturing)


def _round4(n: int) -> int:
    return (n + 3) // 4 * 4


class _Run:
    """At most 64 parameters of a group that step together: their positions in the group, the tensors, the gathered pointers."""
    __slots__ = ("idx", "whole", "params", "states", "pointers", "at")


class _Plan:
    """What a group keeps between steps.  ``params`` is the group's own list (a new list, or a new length, makes a new plan),
    ``members`` the parameters that were in it when the plan was made (another one in a position makes a new plan too)."""
    __slots__ = ("params", "members", "n", "steps", "runs", "state", "state_len", "fresh")


class _FusedOptimizer(torch.optim.Optimizer):
    """What the two optimisers share: the refusals, the closure, and the per-group plans."""

    _REFUSED_FLAGS = ()                 # group keys that must be false / zero

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._plans = {}                # group index -> _Plan

    def __setstate__(self, state):
        super().__setstate__(state)
        self._plans = {}

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans = {}                # (the state dictionaries are new objects)

    @classmethod
    def _check_flags(cls, group) -> None:
        for k in cls._REFUSED_FLAGS:
            if group.get(k):
                raise ValueError(f"{cls.__name__} does not support {k}={group[k]!r}")

    @classmethod
    def _check_param(cls, p) -> None:
        if p.layout != torch.strided:
            raise ValueError(f"{cls.__name__}: parameters must be dense tensors")
        if p.dtype != torch.float32:
            raise ValueError(f"{cls.__name__}: parameters must be float32, got {p.dtype}")
        if not p.is_contiguous():
            raise ValueError(f"{cls.__name__}: parameters must be contiguous, got strides {tuple(p.stride())} for {tuple(p.shape)}")
        if not p.is_cuda:
            raise ValueError(f"{cls.__name__}: parameters must be on the GPU, got {p.device} (use torch's optimiser on the CPU)")

    @staticmethod
    def _closure_loss(closure):
        if closure is None:
            return None
        with torch.enable_grad():
            loss = closure()
        if isinstance(loss, torch.Tensor) and loss.requires_grad:
            raise ValueError("the closure returned a loss that requires grad: return loss.detach() (the graph is not needed "
                             "after backward, and step() would keep it alive)")
        return loss

    def _refuse_capture(self) -> None:
        """What ``step()`` does first when the current stream is capturing (``_cuda_ready() and _capturing()``, inline)."""
        raise RuntimeError(f"{type(self).__name__}.step() cannot be captured into a graph: the step number and lr (lr / bc1, "
                           "sqrt(bc2)) are launch arguments passed by value, so a replay would repeat this step's bias "
                           "corrections and learning rate; call step() outside the capture")

    def _plan(self, gi: int, group, entries: int) -> _Plan:
        """The group's plan, made anew when one of these changed since the last step: the group's list object; its length; the
        identity of a parameter in any position (``group['params'][i] = new_p``, two entries swapped); the optimiser's ``state``
        object; the number of its entries (a state that was cleared, popped from or replaced behind our back).  ``entries`` is
        that number as it was when ``step()`` began, the same for every group: the first step of a parameter adds an entry, and
        one popped since the last step and one added by an earlier group of this step would cancel.  A new plan reads the step
        counts from the state, gives a parameter without state torch's state at step 0 at its first gradient, and leaves the
        state of a parameter that is no longer in the group alone, as torch does."""
        params = group["params"]
        plan = self._plans.get(gi)
        if (plan is None or plan.params is not params or plan.n != len(params) or plan.state is not self.state
                or plan.state_len != entries or not all(map(_is, params, plan.members))):
            plan = self._plans[gi] = _Plan()
            plan.params, plan.members, plan.n, plan.runs = params, tuple(params), len(params), {}
            plan.state, plan.state_len = self.state, len(self.state)
            plan.steps, plan.fresh = None, set()
            self._new_plan(plan)
        return plan

    def _settle(self) -> None:
        """After a step: the number of state entries that the plans were last seen with."""
        for plan in self._plans.values():
            plan.state_len = len(self.state)

    def _new_plan(self, plan) -> None:
        pass

    def _run(self, plan: _Plan, idx) -> _Run:
        """The run of the parameters at positions ``idx`` of the plan's group (a tuple; None: all of them, at most 64)."""
        run = plan.runs.get(idx)
        if run is None:
            if len(plan.runs) >= 64:                # (gradients that come and go in ever new patterns)
                plan.runs.clear()
            run = plan.runs[idx] = _Run()
            run.whole = idx is None
            run.idx = tuple(range(plan.n)) if idx is None else idx
            run.params = [plan.members[i] for i in run.idx]
            run.states = [self.state[p] for p in run.params] if plan.steps is not None else None
            run.pointers = None
            run.at = None
        return run


class FusedAdam(_FusedOptimizer):
    """``torch.optim.Adam`` with ``amsgrad=False``, ``maximize=False`` and L2 (not decoupled) weight decay -- what the reference's
    ``build_optimizer`` constructs -- for float32, contiguous parameters on an MI355X.  ``lr`` is read from the group at every
    ``step()``.  At first use the moments of a group are views of one zero-filled arena each (two fills per group)."""

    _REFUSED_FLAGS = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 capturable=False, differentiable=False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdam: lr must be a number, not a tensor")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # the keys of torch.optim.Adam's groups, so that either class loads the other's state_dict
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=capturable, differentiable=differentiable, fused=None, decoupled_weight_decay=False)
        self._check_flags(defaults)
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._check_flags(group)
            for p in group["params"]:
                self._check_param(p)

    def _new_plan(self, plan) -> None:
        """The group's ``step`` scalars become views of one CPU tensor; a state that is there already (loaded, or from an earlier
        plan) keeps its count -- a number (old checkpoints) or a device tensor (written with ``capturable``) is read once, here."""
        plan.steps = torch.zeros(plan.n, dtype=torch.float32)
        for i, p in enumerate(plan.params):
            st = self.state.get(p)
            if st:
                plan.steps[i] = float(st["step"])
                st["step"] = plan.steps[i]
            else:
                plan.fresh.add(i)

    def _init_state(self, plan, positions) -> None:
        """torch's state at step 0 of the group's parameters at ``positions`` (one device): the moments are views of two
        zero-filled arenas, every view on a 16-byte boundary; ``step`` is the parameter's element of the plan's step tensor."""
        params = [plan.params[i] for i in positions]
        for p in params:
            self._check_param(p)
            if p.device != params[0].device:
                raise ValueError("FusedAdam: the parameters of a group must be on one device")
        total = sum(_round4(p.numel()) for p in params)
        arena_m = torch.zeros(total, dtype=torch.float32, device=params[0].device)
        arena_v = torch.zeros(total, dtype=torch.float32, device=params[0].device)
        at = 0
        for i, p in zip(positions, params):
            n = p.numel()
            st = self.state[p]
            plan.steps[i] = 0.0
            st["step"] = plan.steps[i]
            st["exp_avg"] = arena_m[at:at + n].view(p.shape)
            st["exp_avg_sq"] = arena_v[at:at + n].view(p.shape)
            at += _round4(n)
            plan.fresh.discard(i)

    @staticmethod
    def _moment(st, key, p):
        """``st[key]`` as the contiguous float32 tensor on the parameter's device that the kernel takes (a loaded state is
        whatever torch made of it; anything else is replaced once, in the state itself)."""
        t = st[key]
        if t.dtype != torch.float32 or t.device != p.device or not t.is_contiguous():
            t = st[key] = t.to(device=p.device, dtype=torch.float32).contiguous()
        return t

    def _step_run(self, plan, run, grads, done, group) -> None:
        sts = run.states
        ms = [st["exp_avg"] for st in sts]
        vs = [st["exp_avg_sq"] for st in sts]
        o = run.pointers
        if o is None or o.key != tuple(map(_data_ptr, run.params + ms + vs)):
            for p in run.params:
                self._check_param(p)
            ms = [self._moment(st, "exp_avg", p) for st, p in zip(sts, run.params)]
            vs = [self._moment(st, "exp_avg_sq", p) for st, p in zip(sts, run.params)]
            o = run.pointers = ops.optim_pointers(run.params, ms, vs)
        beta1, beta2 = group["betas"]
        ops.adam_step(run.params, grads, ms, vs, float(group["lr"]), beta1, beta2, group["eps"], group["weight_decay"], done + 1,
                      pointers=o)
        if run.whole:
            plan.steps.add_(1.0)
        else:
            if run.at is None:
                run.at = torch.tensor(run.idx, dtype=torch.long)
            plan.steps.index_add_(0, run.at, torch.ones(len(run.idx)))

    @torch.no_grad()
    def step(self, closure=None):
        if _cuda_ready() and _capturing():
            self._refuse_capture()
        loss = self._closure_loss(closure)
        entries = len(self.state)
        for gi, group in enumerate(self.param_groups):
            self._check_flags(group)
            plan = self._plan(gi, group, entries)
            grads = [p.grad for p in plan.params]
            idx = None                                              # None: every parameter has a gradient
            for g in grads:                                         # (`None in grads` would compare tensors with ==)
                if g is None:
                    idx = tuple(i for i, g in enumerate(grads) if g is not None)
                    break
            if idx == ():
                continue
            if plan.fresh:                                          # the first step of some parameters
                fresh = [i for i in (range(plan.n) if idx is None else idx) if i in plan.fresh]
                for i in fresh:                                     # (later steps: ops.adam_step refuses a sparse gradient)
                    if grads[i].layout is not torch.strided:
                        raise ValueError("FusedAdam does not support sparse gradients")
                if fresh:
                    self._init_state(plan, fresh)
            done = plan.steps.tolist()
            if idx is None and plan.n <= _RUN and done.count(done[0]) == plan.n:         # the normal loop: one launch
                self._step_run(plan, self._run(plan, None), grads, int(done[0]), group)
                continue
            by_step = {}                                                                 # step count -> positions
            for i in (range(plan.n) if idx is None else idx):
                by_step.setdefault(done[i], []).append(i)
            for count, members in by_step.items():
                for at in range(0, len(members), _RUN):
                    run = self._run(plan, tuple(members[at:at + _RUN]))
                    self._step_run(plan, run, [grads[i] for i in run.idx], int(count), group)
        self._settle()
        return loss


class FusedSGD(_FusedOptimizer):
    """``torch.optim.SGD(params, lr)`` -- plain ``p -= lr * grad``, what the reference's ``sgd`` branch constructs -- in one launch
    per group.  No state."""

    _REFUSED_FLAGS = ("momentum", "dampening", "weight_decay", "nesterov", "maximize", "differentiable")

    def __init__(self, params, lr=1e-3, *, maximize=False, differentiable=False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedSGD: lr must be a number, not a tensor")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        # the keys of torch.optim.SGD's groups
        defaults = dict(lr=lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, maximize=maximize, foreach=None,
                        differentiable=differentiable, fused=None)
        self._check_flags(defaults)
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._check_flags(group)
            for p in group["params"]:
                self._check_param(p)

    @torch.no_grad()
    def step(self, closure=None):
        if _cuda_ready() and _capturing():
            self._refuse_capture()
        loss = self._closure_loss(closure)
        entries = len(self.state)
        for gi, group in enumerate(self.param_groups):
            self._check_flags(group)
            plan = self._plan(gi, group, entries)
            grads = [p.grad for p in plan.params]
            idx = tuple(i for i, g in enumerate(grads) if g is not None)
            for at in range(0, len(idx), _RUN):
                members = idx[at:at + _RUN]
                run = self._run(plan, None if len(members) == plan.n else members)
                o = run.pointers
                if o is None or o.key != tuple(map(_data_ptr, run.params)):
                    for p in run.params:
                        self._check_param(p)
                    o = run.pointers = ops.optim_pointers(run.params)
                ops.sgd_step(run.params, [grads[i] for i in run.idx], float(group["lr"]), pointers=o)
        self._settle()
        return loss
