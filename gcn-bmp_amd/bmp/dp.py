"""Data-parallel training step plumbing: one flat fp32 parameter/gradient buffer, ONE RCCL
all-reduce per step, Adam with Chainer's update rule.

Replaces the reference's in-process 2-GPU ``ParallelUpdater`` (train_binary.py:546-549): one
process per GPU, drug pairs sharded by rank, gradients summed with a single ``all_reduce`` over
xGMI (the whole model is 0.3-3 M floats, so the collective is latency-bound and needs no
bucketing or overlap).
"""
from __future__ import annotations

import math
from contextlib import contextmanager
from typing import Optional

import torch
import torch.distributed as dist
from torch import nn
from torch.autograd import Function

from .optim_hooks import HOOK_TYPES, SUMSQ_PARTS_MAX, GradientClipping, Lasso, WeightDecay  # noqa: F401  (re-exported)
from . import optim_hooks as _hooks


class _Unflatten(Function):
    """flat parameter buffer -> the individual parameter tensors (views).  The backward writes all
    parameter gradients into ONE flat tensor with a single concatenation, instead of one
    accumulate kernel per parameter."""

    @staticmethod
    def forward(ctx, flat, shapes):
        ctx.shapes = shapes
        ctx.set_materialize_grads(False)          # unused parameters arrive as None, not as one zero-fill launch each
        outs, off = [], 0
        for shp in shapes:
            n = 1
            for k in shp:
                n *= k
            outs.append(flat[off:off + n].view(shp))
            off += n
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        some = next((g for g in grads if g is not None), None)
        if some is None:
            return None, None
        sizes = []
        for shp in ctx.shapes:
            n = 1
            for k in shp:
                n *= k
            sizes.append(n)
        if all(g is not None for g in grads):
            return torch.cat([g.reshape(-1) for g in grads]), None
        flat = some.new_zeros(sum(sizes))         # parameters the layout plan manages arrive as None: one fill,
        off = 0                                   # then only the autograd-managed slices are copied in
        for g, n in zip(grads, sizes):
            if g is not None:
                flat[off:off + n].copy_(g.reshape(-1))
            off += n
        return flat, None


class FlatAdam:
    """Flattens a module's parameters and gradients into two contiguous buffers (the parameters
    become views) and applies chainer.optimizers.Adam (train_ddi_modify.py:289):
    alpha_t = alpha*sqrt(1-b2^t)/(1-b1^t);  p -= alpha_t*m/(sqrt(v)+eps) + weight_decay_rate*p.
    Chainer's gradient hooks (GradientClipping, WeightDecay, Lasso: bmp.optim_hooks) go in with ``add_hook``.

    ``grad_reduce`` says what the update sees of the ranks' gradients (each the gradient of that rank's mean loss):
    ``"mean"`` (the default) their mean; ``"sum"`` their sum, which is what Chainer's ``ParallelUpdater`` hands to the
    optimizer (``model_main.addgrads(other)``, then ``optimizer.update()``; recalled third-party behaviour, SURVEY.md
    Appendix B).  Adam barely tells the two apart, but the hooks' clip threshold and decay rates act on the one chosen."""

    def __init__(self, module: nn.Module, alpha=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay_rate=0.0,
                 process_group: Optional["dist.ProcessGroup"] = None, grad_reduce: str = "mean"):
        if grad_reduce not in ("mean", "sum"):
            raise ValueError(f"grad_reduce {grad_reduce!r}: 'mean' or 'sum'")
        params = [p for p in module.parameters() if p.requires_grad]
        if not params:
            raise ValueError("module has no parameters")
        if any(isinstance(p, nn.UninitializedParameter) for p in params):
            raise ValueError("the module still has a lazily sized Linear (MLP / SymMLP / HolE built without in_dim / fp_dim): "
                             "call it once, or build it inside GraphConvPredictorForPair, before FlatAdam flattens the parameters")
        dev = params[0].device
        total = sum(p.numel() for p in params)
        self.flat = torch.empty(total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(total, dtype=torch.float32, device=dev)
        off = 0
        for p in params:
            n = p.numel()
            self.flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + n].view_as(p)
            p.grad = self.grad[off:off + n].view_as(p)
            off += n
        self.params = params
        self.names = [n for n, p in module.named_parameters() if p.requires_grad]
        self.shapes = [tuple(p.shape) for p in params]
        self.module = module
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self.t = 0
        self.alpha, self.beta1, self.beta2, self.eps, self.wd = alpha, beta1, beta2, eps, weight_decay_rate
        self.group = process_group
        self.grad_reduce = grad_reduce
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        self.plan = None
        self._plan_tried = False
        self._gscale = 1.0
        self._hooks = {}                    # name -> hook, in the order added
        self._partials = None               # bmp_grad_sumsq_partials' output, allocated with the first clip hook

    def add_hook(self, hook, name: Optional[str] = None) -> None:
        """chainer.Optimizer.add_hook for the hooks of bmp.optim_hooks: they run before the update rule in the order they
        were added.  One hook of each kind; a name (default: the hook's ``name``) may be used once."""
        if not isinstance(hook, HOOK_TYPES):
            raise TypeError(f"FlatAdam runs GradientClipping, WeightDecay and Lasso hooks, not {type(hook).__name__}")
        if any(type(h) is type(hook) for h in self._hooks.values()):
            raise ValueError(f"a {type(hook).__name__} hook is already set")
        name = hook.name if name is None else name
        if name in self._hooks:
            raise KeyError(f"hook {name} already exists")
        if isinstance(hook, GradientClipping) and self.flat.is_cuda and self._partials is None:
            self._partials = torch.empty(SUMSQ_PARTS_MAX, dtype=torch.float32, device=self.flat.device)
        self._hooks[name] = hook

    def remove_hook(self, name: str) -> None:
        del self._hooks[name]

    def hook_order(self) -> int:
        """The kinds of the hooks set, in order (bmp.optim_hooks.hook_order); 0 without hooks."""
        return _hooks.hook_order(self._hooks.values())

    def zero_grad(self) -> None:
        self.grad.zero_()

    # ---- functional mode: one gradient tensor for the whole model, no per-parameter accumulation ----
    def functional_forward(self, *args, **kwargs):
        """Run the module on parameter views produced by ONE autograd node over the flat buffer.
        After ``loss.backward()`` call ``collect_grads()``; the flat gradient is then in ``self.grad``."""
        return self._functional(self.module, args, kwargs)

    def _functional(self, call, args, kwargs):
        leaf = self.flat.detach().requires_grad_()
        self._leaf = leaf
        views = _Unflatten.apply(leaf, self.shapes)
        plan = self._layout_plan()
        hooked = []
        if plan is not None:
            # one launch: every kernel-layout weight array of the planned sub-modules; their weight gradients stay in
            # the plan's buffers until collect_grads()
            plan.prepare(self.flat)
            tape = leaf[:1]
            for prefix, mod in self._plan_sections:
                object.__setattr__(mod, "_fast", (plan.P[prefix], plan.G[prefix], plan.state, tape))   # (nn.Module.__setattr__: 6 us)
                hooked.append(mod)
        # The views stand in for the parameters during the call -- what torch.func.functional_call does, without its
        # per-call walk over the module tree (0.3 ms of host time per step; the RelGCN step is 1.5 ms): every registration
        # of every parameter (tied ones included) was located once.
        slots = self._param_slots()
        try:
            for (reg, key, _orig), k in slots:
                reg[key] = views[k]
            return call(*args, **kwargs)
        finally:
            for (reg, key, orig), _k in slots:
                reg[key] = orig
            for mod in hooked:
                object.__setattr__(mod, "_fast", None)

    def functional_loss(self, *args, t):
        """``functional_forward`` through the module's ``forward_loss`` (GraphConvPredictorForPair: the reference's Classifier,
        train_ddi_modify.py:284-286): the loss of the batch against the labels ``t``, with link predictor + loss as one launch
        each way where the module offers it.  Then ``loss.backward()``, ``collect_grads()``, ``step()`` as usual."""
        return self._functional(lambda *a: self.module.forward_loss(*a, t=t), args, {})

    def functional_predict(self, *args, **kwargs):
        """The evaluation callers' ``predict`` (eval_coattention.py:103-124; training/extensions/batch_evaluator.py:49-100 runs it
        over the train and validation sets every epoch) on the planned path: logits and the two molecule vectors handed to the
        link predictor, under no-backprop.  The kernels then keep nothing for a backward (no m / r|z / c / ij / C stores)."""
        with torch.no_grad():
            y = self.functional_forward(*args, **kwargs)
        return y, (getattr(self.module, "g1", None), getattr(self.module, "g2", None))

    def _param_slots(self):
        """[((module._parameters, name, parameter), index into self.params)] over every registration of a flattened
        parameter in the module tree."""
        if getattr(self, "_slots", None) is None:
            index = {id(p): k for k, p in enumerate(self.params)}
            slots = []
            for mod in self.module.modules():
                for key, prm in mod._parameters.items():
                    if prm is not None and id(prm) in index:
                        slots.append(((mod._parameters, key, prm), index[id(prm)]))
            self._slots = slots
        return self._slots

    def _layout_plan(self):
        """bmp.plan.LayoutPlan over the sub-modules that support it (GGNN encoder, fine co-attention), built at the
        first functional step on a GPU."""
        if self._plan_tried or not self.flat.is_cuda:
            return self.plan
        self._plan_tried = True
        from .plan import LayoutPlan
        sections = []
        for name, mod in self.module.named_modules():
            if name and callable(getattr(mod, "plannable", None)) and mod.plannable() and hasattr(mod, "prepared_layouts"):
                if all(p.requires_grad for p in mod.parameters()):
                    sections.append((name + ".", mod))
        if sections:
            self._plan_sections = sections
            self.plan = LayoutPlan(sections, self.names, self.shapes, self.flat.device)
        return self.plan

    def collect_grads(self) -> None:
        g = self._leaf.grad
        self._leaf = None
        if self.plan is not None:
            if self.plan.state.pop("head_gscale", None) is not None:
                # MLPLossFn.backward handed the factor arriving at the loss to the co-attention node, whose backward did not
                # run (backward(inputs=...) past it, a frozen co-attention): the rows' gradients went on unscaled
                raise RuntimeError("the loss-gradient factor left for the co-attention's backward was never consumed; "
                                   "call loss.backward() through the whole model or use functional_forward + model.loss")
            # one launch: (+)= the planned modules' parameter gradients; when autograd carried none (every parameter is the
            # plan's), that launch writes the whole buffer and no zero-fill precedes it
            self.grad = g if g is not None else torch.empty_like(self.flat)
            self.plan.collect(self.grad, overwrite=g is None)
        else:
            self.grad = g if g is not None else torch.zeros_like(self.flat)

    def reattach(self) -> None:
        """Fold any .grad tensor that autograd (or a caller) replaced back into the flat buffer."""
        off = 0
        for p in self.params:
            n = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.grad[off:off + n].data_ptr():
                if p.grad is not None:
                    self.grad[off:off + n].add_(p.grad.reshape(-1))
                p.grad = self.grad[off:off + n].view_as(p)
            off += n

    def broadcast_parameters(self, src: int = 0) -> None:
        if self.world > 1:
            dist.broadcast(self.flat, src=src, group=self.group)

    def reduce_scale(self) -> float:
        """The factor the update applies to the all-reduced gradient: 1/W for ``grad_reduce="mean"``, 1 for ``"sum"`` and at
        W = 1."""
        return 1.0 / self.world if self.world > 1 and self.grad_reduce == "mean" else 1.0

    def all_reduce_grads(self) -> None:
        """The step's single collective: sum over ranks, then the mean (each rank's loss is the
        mean over its own shard) -- or the sum as it is, with ``grad_reduce="sum"``."""
        if self.world > 1:
            dist.all_reduce(self.grad, op=dist.ReduceOp.SUM, group=self.group)
            scale = self.reduce_scale()
            if scale == 1.0:
                return
            if self.grad.is_cuda:
                self._gscale = scale                 # folded into the Adam kernel
            else:
                self.grad.mul_(scale)

    def step(self) -> None:
        self.t += 1
        a_t = self.alpha * math.sqrt(1.0 - self.beta2 ** self.t) / (1.0 - self.beta1 ** self.t)
        g = self.grad
        if self.flat.is_cuda:                        # the whole update rule as one kernel over the flat buffers
            from . import _lib
            from ._lib import check, ptr, stream
            a_dev = getattr(self, "_alpha_dev", None)        # set by GraphedTrainStep: alpha_t lives on the device there
            if self._hooks:
                self._hooked_step(a_t, a_dev)
                self._gscale = 1.0
                return
            check(_lib.lib().bmp_adam_step(ptr(self.flat), ptr(g), ptr(self.m), ptr(self.v), self.flat.numel(), a_t,
                                           ptr(a_dev), self.beta1, self.beta2, self.eps, self.wd, self._gscale, stream()),
                  "bmp_adam_step")
            self._gscale = 1.0
            return
        if self._hooks:
            g = _hooks.apply_cpu(g, self.flat, self._hooks.values())
        self.m.mul_(self.beta1).add_(g, alpha=1.0 - self.beta1)
        self.v.mul_(self.beta2).addcmul_(g, g, value=1.0 - self.beta2)
        if self.wd:
            self.flat.mul_(1.0 - self.wd)
        self.flat.addcdiv_(self.m, self.v.sqrt().add_(self.eps), value=-a_t)

    def _hooked_step(self, a_t, a_dev) -> None:
        """The hooks and the update on the GPU: the clip's partial sums of squares (when a clip is set), then one launch of
        hooks + Adam.  Their hyperparameters come from the hook objects, or from ``_hook_dev`` (GraphedTrainStep)."""
        from . import _lib
        from ._lib import check, ptr, stream
        hooks = list(self._hooks.values())
        order = _hooks.hook_order(hooks)
        thr, l2, l1 = _hooks.hook_values(hooks)
        h_dev = getattr(self, "_hook_dev", None)
        parts = self._partials if any(h.code == _hooks.CLIP for h in hooks) else None
        n, L, st = self.flat.numel(), _lib.lib(), stream()
        if parts is not None:
            check(L.bmp_grad_sumsq_partials(ptr(parts), ptr(self.grad), ptr(self.flat), n, self._gscale, l2, l1, ptr(h_dev),
                                            order, st), "bmp_grad_sumsq_partials")
        check(L.bmp_adam_step_hooked(ptr(self.flat), ptr(self.grad), ptr(self.m), ptr(self.v), n, a_t, ptr(a_dev), self.beta1,
                                     self.beta2, self.eps, self.wd, self._gscale, thr, l2, l1, ptr(h_dev), order, ptr(parts),
                                     None, st), "bmp_adam_step_hooked")


def shard(n_items: int, rank: int, world: int):
    """Rank r takes items [r*n/W, (r+1)*n/W) of every global batch."""
    per = n_items // world
    return slice(rank * per, (rank + 1) * per)


class GraphedTrainStep:
    """One whole training step (forward, loss, backward, gradient all-reduce, Adam) recorded once per distinct batch -- or
    once for ALL batches of a size, when they are loaded into one ``bmp.packed.StaticPairBatch`` (round 4) -- as a HIP graph
    and replayed: ~55 launches become one submission and the host's per-launch work leaves the step.  Measured: at the reference's default batch of 32
    pairs (train_ddi_modify.py:196) 1.64 -> 1.57 ms per step -- that step is a chain of ~70 dependent kernels of one
    or two workgroup rounds each, bound by their latencies rather than by the host; at 1024 pairs per GPU the step is
    GPU-bound and gains nothing.  Kept as the host-jitter-free way to run a fixed set of batches.

    Everything a replay depends on must sit at fixed device addresses: the packed batch and its labels (device
    resident already), the flat parameter / moment buffers, and Adam's step-dependent factor alpha_t, which is read
    from a one-element device tensor updated before every replay.  Host-side decisions made while recording (which
    gradient buffer a kernel overwrites, which it accumulates into) are the same for every replay of one batch.

    With more than one rank (``opt.world > 1``) a step is recorded as TWO graphs per batch: A = the static batch's
    ``reset_derived`` + ``emit`` (static form), forward, loss, backward and ``collect_grads``; B = the update (the clip's
    partial sums and ``bmp_adam_step_hooked`` with hooks set, ``bmp_adam_step`` without), with the gradient scale of
    ``opt.grad_reduce`` (1/W or 1) fixed in it.  A call replays A, runs ``opt.all_reduce_grads()`` eagerly on the current
    stream -- on the flat gradient A writes and B reads --, then replays B.  The collective stays outside the graphs because
    that is the form both backends run: gloo cannot run inside a recording, and an RCCL all-reduce recorded into a graph has
    never run on this stack.  No collective is issued while a recording is open; the warm-up before recording runs whole
    eager steps, collective included, the same number on every rank.  The replay speed over RCCL is unmeasured.
    """

    def __init__(self, model, opt: "FlatAdam", warmup: int = 2):
        if not opt.flat.is_cuda:
            raise ValueError("graphs need a GPU")
        self.model, self.opt, self.warmup = model, opt, warmup
        self.graphs = {}
        self._alpha = torch.zeros(1, dtype=torch.float32, device=opt.flat.device)
        self._hook_vals = torch.zeros(3, dtype=torch.float32, device=opt.flat.device)     # {threshold, l2, l1}

    def _set_alpha(self) -> None:
        o = self.opt
        self._alpha.fill_(o.alpha * math.sqrt(1.0 - o.beta2 ** (o.t + 1)) / (1.0 - o.beta1 ** (o.t + 1)))
        if o._hooks:                        # the hooks' current thresholds / rates: changed between replays, they still apply
            for k, val in enumerate(_hooks.hook_values(o._hooks.values())):
                self._hook_vals[k].fill_(val)

    @contextmanager
    def _in_line(self):
        plan = self.opt._layout_plan()
        if plan is None:
            yield
            return
        was = getattr(plan, "in_line", False)
        plan.in_line = True                 # one in-order chain: what a replay runs back to back (bmp/plan.py: prepare)
        try:
            yield
        finally:
            plan.in_line = was

    def _body(self, pb, t, static=None):
        with self._in_line():
            loss = self._grads(pb, t, static)
            self.opt.all_reduce_grads()
            self._update()
            return loss

    def _grads(self, pb, t, static=None):
        """Forward, loss, backward, collect_grads: the step up to the flat gradient (graph A at world > 1)."""
        o = self.opt
        if static is not None:
            # a batch at fixed addresses (bmp.packed.StaticPairBatch): its arrays are written by the first launch of the step,
            # and what an earlier step derived from their contents is derived again
            static.reset_derived()
            static.emit()
        if callable(getattr(self.model, "forward_loss", None)):      # the reference's Classifier: link predictor + loss together
            loss = o.functional_loss(pb, t=t)
        else:
            loss = self.model.loss(o.functional_forward(pb), t)
        loss.backward()
        o.collect_grads()
        return loss

    def _update(self) -> None:
        """The hooks and Adam (graph B at world > 1)."""
        o = self.opt
        o._alpha_dev = self._alpha          # Adam reads alpha_t from the device in the recorded step (and only there: eager
        o._hook_dev = self._hook_vals       # steps between replays take it from the host as ever); so do the hooks' values
        try:
            o.step()
        finally:
            o._alpha_dev = None
            o._hook_dev = None

    def __call__(self, pb, t=None) -> torch.Tensor:
        """One step on the batch ``(pb, t)`` -- or on a ``StaticPairBatch`` (``t`` is then its own label array): ONE graph
        (one pair of graphs at world > 1) serves every batch loaded into it."""
        static = pb if callable(getattr(pb, "emit", None)) else None
        if static is not None:
            pb, t = static.pb, static.t
        o = self.opt
        key = (id(pb), id(t), o.hook_order())      # a hook added or removed after recording: a new recording
        if key not in self.graphs:
            # warm-up on a side stream (allocator, lazy builds), with the optimizer state put back afterwards; at world > 1
            # these are whole eager steps, all-reduce included, the same number on every rank
            saved = (o.flat.clone(), o.m.clone(), o.v.clone(), o.t)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(self.warmup):
                    self._set_alpha()
                    self._body(pb, t, static)
            torch.cuda.current_stream().wait_stream(s)
            o.flat.copy_(saved[0]); o.m.copy_(saved[1]); o.v.copy_(saved[2]); o.t = saved[3]
            self.graphs[key] = self._record(pb, t, static)
        rec = self.graphs[key]
        self._set_alpha()
        if o.world == 1:
            g, loss, _pb, _t = rec
            g.replay()
        else:
            ga, gb, loss, grad, _pb, _t = rec
            ga.replay()
            o.grad = grad                       # the flat gradient A writes and B reads (an eager step may have rebound it)
            o.all_reduce_grads()
            o._gscale = 1.0                     # (B holds the scale it was recorded with)
            gb.replay()
        o.t += 1
        return loss

    def _record(self, pb, t, static):
        o = self.opt
        t_before = o.t
        if o.world == 1:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                loss = self._body(pb, t, static)
            o.t = t_before                      # recording does not execute: the step count advances on replay
            return g, loss, pb, t
        ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with self._in_line():
            with torch.cuda.graph(ga):
                loss = self._grads(pb, t, static)
            grad = o.grad
            o._gscale = o.reduce_scale()        # the all-reduce's scale, a launch argument of B's update kernel
            try:
                with torch.cuda.graph(gb):
                    self._update()
            finally:
                o._gscale = 1.0
        o.t = t_before
        return ga, gb, loss, grad, pb, t


class GraphedPredict:
    """The forward-only twin of ``GraphedTrainStep``: the evaluation pass on a ``bmp.packed.StaticPairBatch`` -- the batch's
    ``reset_derived`` + ``emit``, ``opt.functional_predict``, the loss against the batch's labels when a loss function is given,
    and the append of logits, labels, loss and (when asked) the two molecule vectors to a ``bmp.trainer.ScoreSink`` -- recorded
    ONCE as a HIP graph, under ``torch.no_grad()`` with the model in ``eval()``, and replayed for every batch loaded into that
    object.  What the evaluators run over the train and the validation set every epoch (training/extensions/
    batch_evaluator.py:49-100) and the evaluation scripts' ``predict`` (eval_coattention.py:103-124) then cost one submission
    per batch and no host round trip: the sink's append reads its write position from device memory, so every replay lands
    behind the one before, and the set comes to the host in ``sink.finish()``'s one copy.

    ``functional_predict`` calls ``plan.prepare(opt.flat)`` and that launch is part of the recording: a replay after an
    optimizer step sees the new parameters.  The sink's buffers exist, sized, before recording -- their addresses are in the
    graph -- so ``set_sink`` with another sink drops the recordings.  One graph per (batch object, loss function,
    representations); the key is the batch's arrays as in ``GraphedTrainStep``.  The warm-up runs on a side stream and its
    appends are taken back (the sink's three words are restored).  The forward-only path creates nothing per stream: the zero
    word of the fused MLP + loss head (bmp.mlp._ticket) belongs to ``forward_loss``, which an evaluation does not run.

    ``__call__(static)`` returns the logits tensor of the recording, valid until the next replay; with ``sink=None`` it is a
    plain replayed ``predict``.  With ``opt.world > 1`` nothing changes: the forward has no collective, every rank evaluates its
    own share.  The coarse co-attention family (bmp.coarse) reads ``pb.mol_nrows_host`` on the host and sizes tensors by it
    -- sizes read while recording would be frozen into the graph -- so such a model takes the same body eagerly."""

    capacity_hint = None        # (rows, batches) the caller expects to need at most: bmp.trainer sizes a new sink by it

    def __init__(self, model, opt: "FlatAdam", sink=None, warmup: int = 2):
        if not opt.flat.is_cuda:
            raise ValueError("graphs need a GPU")
        self.model, self.opt, self.sink, self.warmup = model, opt, sink, warmup
        self.graphs = {}

    _in_line = GraphedTrainStep._in_line

    def set_sink(self, sink) -> None:
        if sink is not self.sink:
            self.sink = sink
            self.graphs.clear()

    def replays(self) -> bool:
        """False for a model whose forward sizes tensors on the host from the batch's contents (the coarse co-attention family)."""
        return not type(getattr(self.model, "attn", None)).__module__.endswith(".coarse")

    def _body(self, static, lossfun, representations):
        with torch.no_grad(), self._in_line():
            static.reset_derived()
            static.emit()
            y, (g1, g2) = self.opt.functional_predict(static.pb)
            loss = None if lossfun is None else lossfun(y, static.t)
            if representations and (g1 is None or g2 is None):
                raise ValueError("representations: the model leaves no g1 / g2")
            if self.sink is not None:
                self.sink.launch(y, static.t, loss, g1 if representations else None, g2 if representations else None)
            return y, loss, g1, g2

    def __call__(self, static, lossfun=None, representations: bool = False) -> torch.Tensor:
        if not callable(getattr(static, "emit", None)):
            raise ValueError("GraphedPredict runs on a StaticPairBatch (PairBatches(layout='static'))")
        sink = self.sink
        if sink is not None:
            sink.reserve(len(static.t), lossfun is not None)        # the host's capacity check, before any launch
        was_training = self.model.training
        if was_training:                                             # (an evaluation loop has done it: no walk over the modules then)
            self.model.eval()
        try:
            if not self.replays():
                return self._body(static, lossfun, representations)[0]
            lf = (getattr(lossfun, "__func__", lossfun), id(getattr(lossfun, "__self__", None)))
            key = (id(static.pb), id(static.t), lf, bool(representations))
            if key not in self.graphs:
                words = None if sink is None else sink.words.clone()
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    for _ in range(self.warmup):
                        self._body(static, lossfun, representations)
                torch.cuda.current_stream().wait_stream(s)
                if words is not None:
                    sink.words.copy_(words)              # the warm-up's appends never happened
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    outs = self._body(static, lossfun, representations)
                self.graphs[key] = (g, outs, static.pb, static.t, lossfun)
            g, outs = self.graphs[key][:2]
            g.replay()
            return outs[0]
        finally:
            if was_training:
                self.model.train(True)
