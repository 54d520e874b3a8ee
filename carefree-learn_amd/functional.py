"""torch.autograd.Function wrappers: the operator seam of the drop-in.

Each Function replaces one ATen call of the reference's hot path with calls into libcfhip.so and
provides the matching hand-written backward.  Activations are bf16 (what the reference computes
under `mixed_precision="bf16"` autocast), parameters stay fp32 masters with a cached bf16 shadow,
parameter gradients are produced in fp32.

Parameter gradients are written by the backward kernels STRAIGHT into `param.grad` (allocated on
first use, accumulated afterwards) instead of being returned to autograd: that removes one full
read-modify-write pass per parameter and lets the gradient arena / DDP bucket views
(`optim.ParamArena`, `ddp.BucketedAllReduce`) be the kernels' destination.  Because autograd's own
post-accumulate hooks do not fire for such parameters, `grad_ready_callbacks` is invoked instead.
"""
import contextlib
import os
import threading
import weakref
from typing import Any, Callable, Dict, Iterator, List, Optional, Sequence, Tuple

import math

import torch
from torch import Tensor
from torch.autograd import Function

from . import _lib as _lib_mod
from . import ops

bf16 = torch.bfloat16
f32 = torch.float32

# called as cb(param) right after a parameter's gradient has been written by a HIP backward
grad_ready_callbacks: List[Callable[[Tensor], None]] = []
# Called at the top of a backward that re-enters autograd (gradient checkpointing: `torch.autograd.grad` inside
# `_CheckpointFn.backward`), i.e. still in the OUTER graph task: whoever wants an end-of-backward callback of the whole
# pass (ddp.BucketedAllReduce) must queue it from here — queued from a gradient notification inside the nested task it
# would fire when that block's inner backward ends.
backward_entered_callbacks: List[Callable[[], None]] = []
# Weight gradients may be queued for a later grouped launch (fused.queue_linear_dw): whoever is about to consume ALL
# gradients of the pass from an end-of-backward callback of its own (ddp.BucketedAllReduce.finish) calls these first —
# the order in which autograd runs end-of-backward callbacks is the order they were queued in, which is not ours to pick.
deferred_grad_flushes: List[Callable[[], None]] = []


def notify_grad_ready(prm: Tensor) -> None:
    """A HIP backward kernel has been LAUNCHED that leaves `prm.grad` final for this pass: tell the listeners (DDP buckets,
    the optimizer's in-backward ranges).  Recorded by a launch plan (fused.StackPlan) together with the stream it fired on.
    Backwards get here through `commit_grads`."""
    # recording: what the listeners launch themselves (an optimizer range update, a bucket's all-reduce) is THEIR business at
    # replay time too — the plan records the notification, not those launches
    rec = _lib_mod.RECORDER
    if rec is not None:
        _lib_mod.RECORDER = None
    try:
        for cb in grad_ready_callbacks:
            cb(prm)
    finally:
        if rec is not None:
            _lib_mod.RECORDER = rec
    if rec is not None:
        rec.append((2, prm, cur_stream()))


def rec_wait_stream(waiter: "torch.cuda.Stream", waited: "torch.cuda.Stream") -> None:
    waiter.wait_stream(waited)
    if _lib_mod.RECORDER is not None:
        _lib_mod.RECORDER.append((1, waiter.wait_stream, (waited,)))


def rec_wait_event(stream: "torch.cuda.Stream", ev: Any) -> None:
    stream.wait_event(ev)
    if _lib_mod.RECORDER is not None:
        _lib_mod.RECORDER.append((1, stream.wait_event, (ev,)))


def rec_record_event(ev: Any, stream: "torch.cuda.Stream") -> None:
    ev.record(stream)
    if _lib_mod.RECORDER is not None:
        _lib_mod.RECORDER.append((1, ev.record, (stream,)))


# ---------------------------------------------------------------------------------------------
# side HIP stream for the parameter-gradient kernels
# ---------------------------------------------------------------------------------------------
# In backward, dX = dY W (needed by the next layer: the critical path) and dW = dY^T X / db (needed
# only by the optimizer) are independent.  Issuing the dW work on a second HIP stream lets the two
# kernel queues interleave on the CUs: one kernel's store tail and partial last wave of workgroups
# are filled by the other's MFMA work (measured in profiles/).  Inside a hipGraph capture the side
# stream simply becomes a parallel branch of the graph.


# ROCclr multiplexes HIP streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and two streams that share a queue
# run their kernels back to back.  Measured (profiles/r01/rccl_1rank_queues.log + the rocprofv3 queue column): once
# torch.distributed had created its own streams, the dW side stream landed on the compute stream's queue and the step
# lost its overlap (22.9 -> 26.8 ms).  So every helper stream is CHECKED: an idle wavefront on the new stream and on
# each stream it must overlap with, launched together, has to take the time of one; a stream that fails is parked and
# another one is created.  With the check the 1-rank RCCL step is 23.6 ms against 23.1 ms without DDP.  Raising
# GPU_MAX_HW_QUEUES to 8 makes the DDP step SLOWER (27.5 ms, three alternating runs), so the default is left alone.
_SPIN_US = 300
_rejected_streams: List["torch.cuda.Stream"] = []  # kept alive so that their queue slot stays taken
_stream_checks: List[dict] = []  # one record per distinct_stream() call: what stream_report() sums up


def _overlap(streams: List["torch.cuda.Stream"]) -> bool:
    import time

    for st in streams:  # the first launch on a stream creates its queue: not part of the measurement
        with torch.cuda.stream(st):
            ops.spin(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for st in streams:
        with torch.cuda.stream(st):
            ops.spin(_SPIN_US)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) < 1.6e-6 * _SPIN_US


def distinct_stream(others: List["torch.cuda.Stream"], tries: int = 12, priority: int = 0) -> "torch.cuda.Stream":
    """A new stream whose kernels run concurrently with those of every stream in `others` (and of the current one)."""
    base = [torch.cuda.current_stream()] + [st for st in others if st is not None]
    first = None
    for n in range(tries):
        cand = torch.cuda.Stream(priority=priority)
        first = first or cand
        # pairwise against each stream: robust to `others` that already alias one another
        if all(_overlap([st, cand]) for st in base):
            _stream_checks.append(dict(distinct=True, tries=n + 1, against=len(base)))
            return cand
        _rejected_streams.append(cand)
    import warnings

    _stream_checks.append(dict(distinct=False, tries=tries, against=len(base)))
    warnings.warn("cfhip: no helper stream on its own hardware queue after %d tries (GPU_MAX_HW_QUEUES=%s): "
                  "side-stream work will serialise with the compute stream" % (tries, os.environ.get("GPU_MAX_HW_QUEUES")))
    return first


def stream_report() -> dict:
    """What the helper-stream checks of this process found: `distinct` is False as soon as ONE helper stream (batch slice,
    weight-gradient lane, comm stream) had to share a hardware queue with a stream it must overlap with — the step then
    still computes the same numbers, serialised (22.9 -> 26.8 ms when it happened in round 1).  The budget: ROCclr
    multiplexes HIP streams onto GPU_MAX_HW_QUEUES (default 4) hardware queues; the step uses the caller's stream, two
    side lanes (SideStream.lanes) and — data parallel — one comm stream: four."""
    return dict(distinct=all(c["distinct"] for c in _stream_checks), helper_streams=len(_stream_checks),
                tries=max([c["tries"] for c in _stream_checks] or [0]), rejected=len(_rejected_streams),
                max_hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", "default (4)"))


# torch.cuda.current_stream() / torch.cuda.stream(...) walk four Python layers per call (9 / ~20 us); the side-stream
# plumbing below runs ~600 times per UNet step, on the thread that issues every launch.  Same torch entry points, called
# directly (tools/host_profile.py: 14 ms of 65 ms host time per step).
_get_cur = getattr(torch._C, "_cuda_getCurrentStream", None)
_set_cur = getattr(torch._C, "_cuda_setStream", None)
_get_dev = getattr(torch._C, "_cuda_getDevice", None)
_FAST_STREAMS = _get_cur is not None and _set_cur is not None and _get_dev is not None
_cuda_ok: Optional[bool] = None


def cuda_ok() -> bool:
    global _cuda_ok
    if _cuda_ok is None:
        _cuda_ok = torch.cuda.is_available()
    return _cuda_ok


def cur_stream() -> "torch.cuda.Stream":
    """torch.cuda.current_stream() of the current device"""
    if _FAST_STREAMS:
        sid, idx, typ = _get_cur(_get_dev())
        return torch.cuda.Stream(stream_id=sid, device_index=idx, device_type=typ)
    return torch.cuda.current_stream()


class on_stream:
    """`with torch.cuda.stream(side)` without the Python layers (same allocator semantics: tensors created inside belong
    to `side`)."""

    __slots__ = ("side", "prev")

    def __init__(self, side: "torch.cuda.Stream") -> None:
        self.side = side
        self.prev = None

    def __enter__(self) -> None:
        if _FAST_STREAMS:
            self.prev = _get_cur(_get_dev())
            _set_cur(stream_id=self.side.stream_id, device_index=self.side.device_index, device_type=self.side.device_type)
        else:
            self.prev = torch.cuda.current_stream()
            torch.cuda.set_stream(self.side)

    def __exit__(self, *exc: Any) -> None:
        if _FAST_STREAMS:
            _set_cur(stream_id=self.prev[0], device_index=self.prev[1], device_type=self.prev[2])
        else:
            torch.cuda.set_stream(self.prev)


# HIP stream priority per side lane (A/B knob: CFHIP_LANE_PRIORITY="0:-1,1:0"; negative = higher priority)
LANE_PRIORITY: dict = {}  # lane -> HIP stream priority; measured flat (profiles/r05, tools/gpu/lane_priority_ab.sh): a variable for A/B scripts, no environment switch since round 6


class SideStream:
    enabled = True
    # side streams: lane 0 carries the weight-gradient launches (and the forward's second batch slice), lane 1 the backward's
    # second batch slice.  TWO, not more: with the caller's stream and the comm stream of a data-parallel run that is the four
    # hardware queues ROCclr has by default — a third lane (three batch slices measured slower anyway) left the comm stream
    # without a queue of its own in every ProcessGroup run of round 3.  fused.py raises it when
    # CFHIP_FWD_HALVES / CFHIP_BWD_HALVES ask for more slices.
    lanes = 2
    heavy = True  # False: the dW GEMMs stay on the caller's stream, only the small reductions go aside
    streams: List[Optional["torch.cuda.Stream"]] = [None, None, None, None]
    keep: List[Tensor] = []  # operands produced on the main stream, alive until the join

    _join_queued = False

    @classmethod
    def get(cls, lane: int = 0) -> "torch.cuda.Stream":
        """The side stream of a lane; created (and checked for its own hardware queue) on first use."""
        lane = lane % max(1, cls.lanes)
        if cls.streams[lane] is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("cfhip: side streams must exist before a hipGraph capture starts (run one eager step)")
            cls.streams[lane] = distinct_stream(cls.streams, priority=LANE_PRIORITY.get(lane, 0))
        return cls.streams[lane]

    @classmethod
    def ensure(cls) -> None:
        for lane in range(max(1, cls.lanes)):
            cls.get(lane)

    @classmethod
    def _end_of_backward(cls) -> None:
        cls._join_queued = False
        cls.join()

    @classmethod
    def run(cls, fn: Callable[[], None], keep: Tuple[Tensor, ...] = (), lane: int = 0,
            wait: Tuple["torch.cuda.Stream", ...] = ()) -> None:
        """`fn` on the side stream of `lane`, ordered after the current stream and after every stream in `wait`
        (operands written by other streams, e.g. the second batch slice of the backward pass)."""
        if not cls.enabled or not cuda_ok() or (lane == 0 and not cls.heavy):
            for st in wait:
                cur_stream().wait_stream(st)
            fn()
            return
        if not cls._join_queued:
            # join automatically when the running backward pass ends, so that whoever reads `.grad`
            # afterwards on the caller's stream is ordered after the side-stream kernels
            try:
                torch.autograd.Variable._execution_engine.queue_callback(cls._end_of_backward)
                cls._join_queued = True
            except RuntimeError:  # not inside a backward pass: stay on the current stream
                for st in wait:
                    cur_stream().wait_stream(st)
                fn()
                return
        side = cls.get(lane)
        rec_wait_stream(side, cur_stream())  # everything issued so far is visible
        for st in wait:
            if st is not side:
                rec_wait_stream(side, st)
        with on_stream(side):
            fn()
        cls.keep.extend(keep)

    @classmethod
    def fork(cls, lane: int = 0) -> Optional["torch.cuda.Stream"]:
        """A side stream that has waited for the current stream (for work the caller joins itself)."""
        if not cls.enabled or not cuda_ok():
            return None
        side = cls.get(lane)
        rec_wait_stream(side, cur_stream())
        return side

    @classmethod
    def queue_join(cls) -> None:
        """A replayed backward (fused.StackPlan) put work on the side lanes without going through `run`: make sure the
        running backward pass ends with the join."""
        if not cls._join_queued:
            try:
                torch.autograd.Variable._execution_engine.queue_callback(cls._end_of_backward)
                cls._join_queued = True
            except RuntimeError:
                pass

    @classmethod
    def join(cls) -> None:
        """Make the current stream wait for the side stream (call before consuming parameter grads)."""
        for side in cls.streams:
            if side is not None:
                cur_stream().wait_stream(side)
        cls.keep.clear()


# ---------------------------------------------------------------------------------------------
# Taped composite nodes (round 5): a whole sub-module as ONE autograd node
# ---------------------------------------------------------------------------------------------
# The composed module paths (the UNet's residual block and spatial transformer: residual.py:154-253, mixed_stacks/api.py:766-893)
# are chains of the Functions of this file.  Through autograd each link costs a `Function.apply` on the way in and an engine
# dispatch on the way back (8-9 us of host time each, ~600 links per zoo-UNet step whose forward is bound by the host's issue
# rate) and every fan-in is an ATen add.  Inside a taped node the SAME static `forward` / `backward` of every Function run
# against a plain context object: `TapedFn.forward` records (Function, context, argument slots) while the module's own forward
# code runs, `TapedFn.backward` walks the record in reverse, sums fan-ins with `cfhip_add_bf16` and lets LayerNorm's backward
# kernel take the gradient its input has already received as its `dx_add` operand.  Nothing is re-implemented per module.
# What the tape cannot see is a plain torch op BETWEEN two Functions (its result would silently drop out of the gradient):
# views of taped tensors are detected and end the attempt (`TapeBreak`: the module runs its composed path from then on); the
# modules that use the tape only do so for configurations whose op sequence is known to consist of Functions
# (tests/test_gpu_unet.py compares every gradient of both node types with the composed path).
# MEASURED (profiles/r05/unet_taped_nodes.txt): the zoo UNet's graph shrinks from 1 201 to 751 autograd nodes, the host's backward
# from ~28 to ~24-29 ms, its forward GROWS from 14.5 to 17-18 ms (collecting a node's parameters and slots costs more than the
# `apply` calls it saves) — and neither matters: the GPU needs 19.1 ms for the forward and 39.8 ms for the backward either way
# (events around the phases), so the step is bound by the queues in BOTH phases, 59.7 vs 59.6-60.0 ms.  Off by default.

TAPED_NODES = [os.environ.get("CFHIP_TAPED_NODES", "0") == "1"]  # built, measured, not selected: see the note below
_TAPE = threading.local()  # `.tape`: the tape that records on THIS thread (a forward on another thread is none of its business)


class TapeBreak(RuntimeError):
    """the sub-module's forward did something the tape cannot differentiate"""


class _TapeCtx:
    """what a Function's static `forward` / `backward` get in place of autograd's context while a tape records"""

    def __init__(self, needs: Tuple[bool, ...]):
        self.needs_input_grad = needs
        self.saved_tensors: Tuple[Any, ...] = ()

    def save_for_backward(self, *tensors: Any) -> None:
        self.saved_tensors = tensors

    def set_materialize_grads(self, value: bool) -> None:
        pass

    def mark_non_differentiable(self, *tensors: Any) -> None:
        pass


class _Tape:
    def __init__(self, inputs: Tuple[Any, ...]):
        self.n_inputs = len(inputs)
        self.by_id = {id(t): i for i, t in enumerate(inputs) if isinstance(t, Tensor) and t.requires_grad}
        self.inputs = inputs  # keeps the ids stable
        self.entries: List[Tuple[Any, _TapeCtx, Tuple[Any, ...], int]] = []
        self.next_slot = len(inputs)
        self.out_slot = -1
        self.used = False
        self.token = object()  # what taped results carry (not the tape itself: a result saved by its own link would close a cycle)

    def slot(self, t: Tensor) -> Optional[Tuple[int, Optional[torch.Size]]]:
        """(slot, None) of a node input or a taped result; (slot, parameter shape) of a contiguous view of a whole parameter;
        None for a constant"""
        s = getattr(t, "_cfhip_slot", None)
        if s is not None and s[0] is self.token:
            return s[1], None
        i = self.by_id.get(id(t))
        if i is not None:
            return i, None
        if t._is_view():
            base = t._base
            i = None if base is None else self.by_id.get(id(base))
            if (i is not None and base.is_leaf and base.numel() == t.numel() and t.is_contiguous() and base.is_contiguous()
                    and t.data_ptr() == base.data_ptr()):
                return i, base.shape  # e.g. a [Cout, Cin, 1, 1] filter seen as the matrix of its GEMM (cf. whole_param)
            if base is not None and (i is not None or (getattr(base, "_cfhip_slot", None) or (None,))[0] is self.token):
                raise TapeBreak("a view of a taped tensor reached a Function: the tape has no gradient rule for the view")
        return None

    def record(self, fn: Any, args: Tuple[Any, ...]) -> Any:
        slots = tuple(self.slot(a) if isinstance(a, Tensor) else None for a in args)
        ctx = _TapeCtx(tuple(sl is not None for sl in slots))
        out = fn.forward(ctx, *args)
        if any(sl is not None for sl in slots):
            if not isinstance(out, Tensor):
                raise TapeBreak(f"{fn.__name__} returns {type(out).__name__}: only single-tensor Functions are taped")
            if any(out is a for a in args):  # an identity link: its result needs an identity of its own
                out = out.view_as(out)
            out._cfhip_slot = (self.token, self.next_slot)
            metas = tuple(None if sl is None else (sl[0], sl[1], a.dtype, a.shape) for sl, a in zip(slots, args))
            self.entries.append((fn, ctx, metas, self.next_slot))
            self.next_slot += 1
        return out

    def backward(self, dy: Tensor) -> List[Optional[Tensor]]:
        if self.used:
            raise RuntimeError("cfhip: a taped node was differentiated twice (retain_graph / double backward); set "
                               "CFHIP_TAPED_NODES=0 or functional.TAPED_NODES[0] = False for such a graph")
        self.used = True
        grads: dict = {self.out_slot: dy}
        entries = self.entries
        while entries:
            fn, ctx, metas, out_slot = entries.pop()  # popped: what the link saved is freed as the walk passes it
            g = grads.pop(out_slot, None)
            if g is None:
                continue
            first = metas[0]
            if getattr(fn, "folds_dx_add", False) and first is not None and first[1] is None:
                pending = grads.get(first[0])
                if pending is not None and pending.dtype == bf16 and pending.shape == first[3] and pending.is_contiguous():
                    ctx.dx_add = grads.pop(first[0])  # the kernel adds it: the link's dx then IS the sum so far
            gin = fn.backward(ctx, g)
            if not isinstance(gin, tuple):
                gin = (gin,)
            for meta, ga in zip(metas, gin):
                if meta is None or ga is None:
                    continue
                slot, param_shape, dtype, shape = meta
                if ga.shape != shape:
                    raise RuntimeError(f"cfhip taped node: {fn.__name__}.backward returned {tuple(ga.shape)} for an input of {tuple(shape)}")
                if ga.dtype != dtype:
                    ga = ga.to(dtype)  # what autograd's engine does between two nodes
                if param_shape is not None:
                    ga = ga.reshape(param_shape)
                prev = grads.get(slot)
                grads[slot] = ga if prev is None else _sum_grads(prev, ga)
        self.inputs = ()
        return [grads.get(i) for i in range(self.n_inputs)]


def _sum_grads(a: Tensor, b: Tensor) -> Tensor:
    if a.dtype == bf16 and b.dtype == bf16 and a.is_cuda and a.shape == b.shape:
        return AddFn.forward(None, a, b)  # a new tensor: either operand may be somebody else's gradient too
    return a + b


def _apply(fn: Any, *args: Any) -> Any:
    """`fn.apply(*args)`, or — inside a taped node — the Function's forward run directly and put on the tape"""
    tape = getattr(_TAPE, "tape", None)
    if tape is None:
        return fn.apply(*args)
    if not getattr(fn, "tapeable", True):
        raise TapeBreak(f"{fn.__name__} cannot run inside a taped node")
    return tape.record(fn, args)


class TapedFn(Function):
    @staticmethod
    def forward(ctx: Any, run: Callable[[], Tensor], *tensors: Any) -> Tensor:
        tape = _Tape(tensors)
        _TAPE.tape = tape
        try:
            out = run()
        finally:
            _TAPE.tape = None
        s = getattr(out, "_cfhip_slot", None)
        if s is None or s[0] is not tape.token:
            raise TapeBreak("the sub-module's result is not the result of a taped Function")
        tape.out_slot = s[1]
        ctx.tape = tape
        return out

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        return (None,) + tuple(ctx.tape.backward(dy))


def run_taped(run: Callable[[], Tensor], tensors: Tuple[Any, ...]) -> Tensor:
    """`run()` as one autograd node over `tensors` (the activations it reads and every parameter it uses); plainly when a tape is
    already recording (nested sub-modules join the outer node), without grad mode, or when nothing asks for a gradient."""
    if getattr(_TAPE, "tape", None) is not None or not torch.is_grad_enabled():
        return run()
    return TapedFn.apply(run, *tensors)


# ---------------------------------------------------------------------------------------------
# bf16 shadows of fp32 master parameters
# ---------------------------------------------------------------------------------------------


def shadow_bf16(param: Tensor) -> Tensor:
    """bf16 copy of an fp32 parameter, re-cast only when the parameter changed.

    `optim.ParamArena` installs arena-backed shadows that its fused Adam kernel refreshes in the
    same pass that updates the master weights; otherwise the copy is keyed on `param._version`.
    """
    if param.dtype == bf16:
        return param.detach()
    sh = getattr(param, "_cfhip_shadow", None)
    ver = param._version
    if sh is not None and getattr(param, "_cfhip_shadow_version", None) == ver and sh.device == param.device:
        return sh
    src = param.detach()
    if sh is None or sh.shape != src.shape or sh.device != src.device:
        sh = torch.empty(src.shape, dtype=bf16, device=src.device)
    ops.to_bf16(src.contiguous(), out=sh)
    try:
        param._cfhip_shadow = sh
        param._cfhip_shadow_version = ver
    except Exception:  # non-leaf views etc.: just do not cache
        pass
    return sh


def _is_direct(param: Optional[Tensor]) -> bool:
    return param is not None and param.is_leaf and param.requires_grad and param.dtype == f32


def whole_param(t: Optional[Tensor]) -> Optional[Tensor]:
    """`t` itself, or — when `t` is a contiguous view of a WHOLE leaf parameter (a [Cout, Cin, 1, 1] filter seen as the
    [Cout, Cin] matrix of the GEMM it is) — that parameter: its gradient can then be written straight into `.grad` (and
    run on the side stream) instead of travelling back through autograd's view chain."""
    if t is None or not t._is_view():
        return t
    # A view taken WITHOUT grad mode is a leaf that does not require grad.  Inside a taped node (TapedFn.forward runs without grad
    # mode) that is the normal case and the view stands for its parameter; anywhere else it is a weight somebody froze on purpose
    # (a view cached under torch.no_grad()): it must not resolve to its base and silently receive gradients / optimizer updates
    # (ADVICE r5).
    if t.is_leaf and getattr(_TAPE, "tape", None) is None:
        return t
    base = t._base
    if (base is not None and base.is_leaf and base.requires_grad and base.dtype == f32 and base.numel() == t.numel()
            and t.is_contiguous() and base.is_contiguous() and t.data_ptr() == base.data_ptr()):
        return base
    return t


def grad_buffer(param: Tensor, zero: bool = False) -> Tensor:
    """The tensor a backward kernel writes `param`'s gradient into when `param.grad is None`: the parameter's slot of
    its `optim.ParamArena` when it lives in one (the reference trainer's `optimizer.zero_grad()` sets `.grad` to None
    every step; the bucketed all-reduce and the fused Adam read the arena), a new tensor otherwise.  Contents are
    undefined unless `zero`."""
    arena = getattr(param, "_cfhip_arena", None)
    if arena is not None:
        buf = arena.grad_view(param)
        if zero:
            buf.zero_()
        return buf
    make = torch.zeros if zero else torch.empty
    return make(param.shape, dtype=f32, device=param.device)


# ---- the direct-write protocol: claim (where does the kernel write, does it overwrite or add) -> launch -> commit --------------
# `optim.ParamArena` owns the other half: `zero_grad(lazy)` sets the 'fresh' mark, `_fresh_guard` / `finalize_grads` consume it.


def claim_grads(params: Sequence[Tensor], zero_new: bool = False) -> List[Tuple[Tensor, bool]]:
    """(destination, accumulate) for each parameter a backward kernel is about to write: a `.grad` that is None comes back as
    `grad_buffer(param)` and is written; one that carries the 'fresh' mark of a lazy zero-grad holds last step's values and is
    written too; anything else is accumulated into.  `zero_new`: a `.grad` that was None comes back ZEROED and is accumulated
    into instead — `PatchTokensFn` alone asks for it; its kernel overwrites every element it owns, so the memset buys nothing,
    but it has always been part of that backward's launch sequence and stays there."""
    out = []
    for prm in params:
        if prm.grad is None:
            prm.grad = grad_buffer(prm, zero=zero_new)
            prm._cfhip_fresh = not zero_new
        out.append((prm.grad, not getattr(prm, "_cfhip_fresh", False)))
    return out


def claim_grads_one_flag(params: Sequence[Tensor], zero_new: bool = False) -> Tuple[List[Tensor], bool]:
    """`claim_grads` for ONE kernel that takes one accumulate flag for all its destinations (LayerNorm's dgamma / dbeta, the
    head token / positional table).  When some are to be written and others accumulated into, the ones to be written are
    zeroed and the kernel accumulates into all of them: the same sums, one memset more, in a state (a pair whose members
    were zeroed at different times) that no training step of this package produces."""
    claims = claim_grads(params, zero_new)
    acc = any(a for _, a in claims)
    if acc:
        for buf, a in claims:
            if not a:
                buf.zero_()
    return [buf for buf, _ in claims], acc


def commit_grads(params: Sequence[Tensor], notify: bool = True) -> None:
    """The kernel that leaves these gradients final for this pass has been LAUNCHED: later writes of the pass accumulate, and
    the listeners are told (`notify=False`: a batch-sliced backward tells them once, after the last slice has added its rows)."""
    for prm in params:
        prm._cfhip_fresh = False
        if notify:
            notify_grad_ready(prm)


def write_param_grad(param: Tensor, compute: Callable[[Tensor, bool], None]) -> None:
    """`compute(out, accumulate)` must write (accumulate=False) or add (True) the f32 gradient."""
    ((buf, acc),) = claim_grads((param,))
    compute(buf, acc)
    commit_grads((param,))


def write_param_grad_pair(a: Tensor, b: Tensor, compute: Callable[[Tensor, Tensor, bool], None]) -> None:
    """Two gradients that ONE kernel writes with one accumulate flag (LayerNorm's dgamma / dbeta): `compute(out_a, out_b,
    accumulate)`."""
    (ga, gb), acc = claim_grads_one_flag((a, b))
    compute(ga, gb, acc)
    commit_grads((a, b))


def param_grad(param: Tensor, compute: Callable[[Tensor, bool], None]) -> Optional[Tensor]:
    """`write_param_grad` when the gradient goes straight into `.grad` (None for autograd), else a new tensor that `compute`
    has written, for autograd to accumulate."""
    if _is_direct(param):
        write_param_grad(param, compute)
        return None
    g = torch.empty(param.shape, dtype=f32, device=param.device)
    compute(g, False)
    return g


def grads_in_one_launch(params: Dict[str, Tensor], launch: Callable[[Dict[str, Tensor], List[str]], None]) -> Dict[str, Optional[Tensor]]:
    """`launch(dests, accumulate)` runs once with a destination for every parameter of `params` (name -> parameter that asks for a
    gradient), each claimed through `functional.param_grad`: the claims nest, the innermost one launches, and every commit (which tells
    the in-backward optimizer) happens after the launch.  Returns name -> what autograd gets (None for a direct `.grad` write)."""
    names = list(params)
    dests: Dict[str, Tensor] = {}
    accumulate: List[str] = []
    results: Dict[str, Optional[Tensor]] = {}

    def level(i: int) -> None:
        if i == len(names):
            launch(dests, accumulate)
            return
        name = names[i]

        def compute(out: Tensor, acc: bool) -> None:
            dests[name] = out
            if acc:
                accumulate.append(name)
            level(i + 1)

        results[name] = param_grad(params[name], compute)

    level(0)
    return results


def store_param_grad(param: Tensor, g: Tensor) -> Optional[Tensor]:
    """A gradient that already exists as a tensor: added to / copied into `.grad` (None for autograd), or handed to autograd."""
    if _is_direct(param):
        write_param_grad(param, lambda out, acc: out.add_(g.view(out.shape)) if acc else out.copy_(g.view(out.shape)))
        return None
    return g.view(param.shape)


def _as_rows(x: Tensor) -> Tensor:
    """[..., D] -> 2-D view with a contiguous last dim, keeping f32 or bf16 as is."""
    x2 = x.reshape(-1, x.shape[-1])
    if x2.dtype not in (bf16, f32):
        x2 = x2.float()
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    return x2


def _as_bf16_2d(x: Tensor) -> Tensor:
    x2 = x.reshape(-1, x.shape[-1])
    if x2.dtype != bf16:
        x2 = ops.to_bf16(x2.float() if x2.dtype != f32 else x2)
    if x2.stride(-1) != 1 or (x2.dim() == 2 and x2.stride(0) % 8 != 0 and x2.shape[0] > 1):
        x2 = x2.contiguous()
    return x2


# ---------------------------------------------------------------------------------------------
# Linear (K1): y = x W^T + b, optional fused GELU / residual-add epilogue
# ---------------------------------------------------------------------------------------------

ACT_NONE, ACT_GELU, ACT_QGELU = 0, 1, 2


def _all_direct(weight: Tensor, bias: Optional[Tensor]) -> bool:
    """Every gradient this op owes is written straight into an arena-owned `.grad` (nothing is returned to autograd)."""
    if weight.requires_grad and not _is_direct(weight):
        return False
    return bias is None or not bias.requires_grad or _is_direct(bias)


def _linear_param_grads(dy2: Tensor, x2: Tensor, weight: Tensor, bias: Optional[Tensor]) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """dW = dy^T x, db = colsum(dy): direct-to-.grad when possible, returned otherwise."""
    gw = gb = None
    n, k, m = dy2.shape[1], x2.shape[1], x2.shape[0]  # (the parameter may be a [n, k, 1, 1] filter: whole_param)
    fast_ok = dy2.shape[1] % 8 == 0 and x2.shape[1] % 8 == 0 and dy2.stride(0) % 8 == 0 and x2.stride(0) % 8 == 0
    # split-K lives on the MFMA path only; narrow tabular heads (3 classes, 10 features) take the shape-agnostic kernel
    split = ops.pick_split_k(n, k, m) if fast_ok else 1

    def dw_into(out: Tensor, acc: bool) -> None:
        ops.gemm(dy2, x2, a_trans=True, b_trans=True, out=out.view(n, k), accumulate=acc, split_k=split)

    if _is_direct(weight) and _is_direct(bias) and fast_ok:
        from .fused import _dw_db  # one launch for dW and db

        _dw_db(weight, bias, dy2, x2)
        return None, None
    if weight.requires_grad:
        gw = param_grad(weight, dw_into)
    if bias is not None and bias.requires_grad:
        gb = param_grad(bias, lambda out, acc: ops.colsum(dy2, out=out.view(-1), accumulate=acc))
    return gw, gb


linear_param_grads = _linear_param_grads  # for the Functions of other modules that hold a Linear layer's GEMMs themselves (rwkv.py)


# ---- fan-in links (round 6; VERDICT r5 #3b "fan-in adds inside the consumer") -----------------------------------------------------------
# `net = f(LN(net)) + net` with the add riding in the last GEMM's epilogue (the UNet's SpatialTransformerBlock, three times per block):
# in backward the GEMM's Function returns dY for the residual operand, the LayerNorm's returns dx, and autograd's engine sums the two with an
# ATen add (45 launches and 1.7 GB of traffic per 64^2 x 8 step).  Inside a `fanin_links()` scope a LayerNormFn that sees a bf16 input
# requiring a gradient leaves a link behind; a LinearFn whose `residual` operand IS that tensor takes the link, and in backward hands its dY
# to the link instead of to autograd (None for the residual); the LayerNorm backward — which runs later, it sits upstream of that GEMM —
# passes it to its kernel as `dx_add`: one rounding instead of two, no add launch.  The scope is the module's promise that the GEMM consumes
# (a function of) that LayerNorm's output, i.e. that the LayerNorm backward runs after, and whenever, the GEMM's does.
FANIN_LINKS = True  # (A/B: tools set the attribute)


class FanInLink:
    __slots__ = ("pending", "__weakref__")

    def __init__(self) -> None:
        self.pending: Optional[Tensor] = None


class _FanInState(threading.local):
    def __init__(self) -> None:
        self.active = 0
        self.entries: List[Tuple[Any, FanInLink]] = []


_FANIN = _FanInState()


@contextlib.contextmanager
def fanin_links():
    if not FANIN_LINKS:
        yield
        return
    _FANIN.active += 1
    try:
        yield
    finally:
        _FANIN.active -= 1
        if _FANIN.active == 0:
            _FANIN.entries.clear()


def _fanin_offer(ctx: Any, x: Tensor) -> None:
    """LayerNormFn.forward: leave a link for the GEMM that will add `x` back"""
    ctx.link = None
    if _FANIN.active and x.dtype == bf16 and getattr(_TAPE, "tape", None) is None and ctx.needs_input_grad[0]:
        ctx.link = FanInLink()
        _FANIN.entries.append((weakref.ref(x), ctx.link))
        del _FANIN.entries[:-4]


def _fanin_take(residual: Optional[Tensor]) -> Optional[FanInLink]:
    """LinearFn.forward: the link of the LayerNorm that read this very tensor, if one is waiting"""
    if residual is None or not _FANIN.active or residual.dtype != bf16:
        return None
    for i, (ref, link) in enumerate(_FANIN.entries):
        if ref() is residual:
            del _FANIN.entries[i]
            return link
    return None


class LinearFn(Function):
    """Replaces F.linear (reference customs.py:89, attentions.py:214) incl. backward."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, weight: Tensor, bias: Optional[Tensor], act: int,
                residual: Optional[Tensor], out_f32: bool) -> Tensor:
        x2 = _as_bf16_2d(x)
        wshape = weight.shape
        weight, bias = whole_param(weight), whole_param(bias)
        w16 = shadow_bf16(weight).view(wshape)
        bias_f = None if bias is None else bias.detach().reshape(-1).contiguous()
        m, n = x2.shape[0], wshape[0]
        pre = None
        if act in (ACT_GELU, ACT_QGELU):
            pre = torch.empty((m, n), dtype=bf16, device=x2.device)
            y = ops.gemm(x2, w16, bias=bias_f, epilogue=ops.EPI_GELU if act == ACT_GELU else ops.EPI_QGELU,
                         aux_out=pre)
        elif residual is not None:
            # the residual operand keeps its dtype: an f32 residual stream gives an f32 sum
            r2 = _as_rows(residual)
            if not r2.is_contiguous():
                r2 = r2.contiguous()
            y = ops.gemm(x2, w16, bias=bias_f, epilogue=ops.EPI_RESIDUAL, aux_in=r2, out_dtype=r2.dtype)
        else:
            y = ops.gemm(x2, w16, bias=bias_f, out_dtype=f32 if out_f32 else bf16)
        ctx.save_for_backward(x2, w16, pre)
        ctx.weight, ctx.bias = weight, bias
        ctx.n = n
        ctx.has_residual = residual is not None
        ctx.link = _fanin_take(residual) if residual is not None and y.dtype == bf16 else None
        ctx.x_shape = x.shape
        ctx.in_dtype = x.dtype
        ctx.act = act
        return y.view(*x.shape[:-1], n)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        x2, w16, pre = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        dy2 = _as_bf16_2d(dy)
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        d_res = dy2.view(*ctx.x_shape[:-1], ctx.n) if ctx.has_residual and ctx.needs_input_grad[4] else None
        # (autograd casts d_res to the residual's dtype; the gradient stream itself stays bf16)
        link = getattr(ctx, "link", None)
        if link is not None and d_res is not None:  # the LayerNorm that read the residual operand adds it inside its backward kernel
            link.pending, d_res = dy2, None
        if pre is not None:
            dy2 = ops.gelu_bwd(dy2, pre) if ctx.act == ACT_GELU else ops.quick_gelu_bwd(dy2, pre)
        gw = gb = None
        if _all_direct(weight, bias):
            # gradients that land straight in `.grad` do not go back through autograd: they run on the side stream,
            # beside the dX GEMM below (issued first so that the side stream does not wait for dX)
            from . import fused  # (round 3) weight gradients of stand-alone Linear layers join the grouped launches

            if not fused.queue_linear_dw(weight, bias, dy2, x2):
                SideStream.run(lambda: _linear_param_grads(dy2, x2, weight, bias), (dy2, x2))
            dx = ops.gemm(dy2, w16, b_trans=True).view(ctx.x_shape) if ctx.needs_input_grad[0] else None
        else:
            dx = None
            if ctx.needs_input_grad[0]:
                dx = ops.gemm(dy2, w16, b_trans=True).view(ctx.x_shape)  # bf16; autograd casts if needed
            gw, gb = _linear_param_grads(dy2, x2, weight, bias)
        return dx, gw, gb, None, d_res, None


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, *, act: int = ACT_NONE,
           residual: Optional[Tensor] = None, out_f32: bool = False) -> Tensor:
    return _apply(LinearFn, x, weight, bias, act, residual, out_f32)


# ---------------------------------------------------------------------------------------------
# Linear with a LoRA adapter: act(x W^T + b [+ residual] + s * drop(x A^T Bm^T)) — the reference's LoRALinearHook in training mode
# (hijacks.py:42-49,157-166: the low-rank term is added to the Linear's output, i.e. BEFORE any activation that follows it)
# ---------------------------------------------------------------------------------------------


class _PhiloxCarry(threading.local):
    """(seed, offset) pairs drawn inside a `gradient_checkpoint`ed function: recorded by the no-grad forward, handed out again, in
    order, to the recomputation inside backward — the recomputed masks are the ones the forward's output was made with."""

    def __init__(self) -> None:
        self.record: Optional[List[Tuple[int, int]]] = None
        self.replay: Optional[Iterator[Tuple[int, int]]] = None


_PHILOX = _PhiloxCarry()


def take_philox(counters: int) -> Tuple[int, int]:
    """`ops.PhiloxState.take`, repeatable under `gradient_checkpoint` (see _PhiloxCarry)"""
    st = _PHILOX
    if st.replay is not None:
        try:
            pair = next(st.replay)
        except StopIteration:
            raise RuntimeError("cfhip: the recomputation of a checkpointed function drew more dropout masks than its forward did") from None
    else:
        pair = ops.PhiloxState.take(counters)
    if st.record is not None:
        st.record.append(pair)
    return pair


class LoRALinearFn(Function):
    """Base GEMM (bias / residual epilogues kept, no activation epilogue) -> ops.lora_down -> ops.lora_up_add on the GEMM's output ->
    the stand-alone GELU / quick-GELU kernel, which saves the pre-activation as LinearFn does.  `scale` is a host float (hook.scale *
    alpha / rank, read once per set_scale / load_state_dict: no device sync here); `p` the dropout rate on the low-rank term, its mask
    regenerated in backward from the (seed, offset) the forward drew.  A frozen base launches neither dW nor db."""

    tapeable = False  # a hooked layer never sits inside a taped node (modules._plain_children)

    @staticmethod
    def forward(ctx: Any, x: Tensor, weight: Tensor, bias: Optional[Tensor], A: Tensor, Bm: Tensor, scale: float, p: float,
                act: int, residual: Optional[Tensor], out_f32: bool) -> Tensor:
        if act != ACT_NONE and residual is not None:
            raise ValueError("LoRALinearFn: an activation and a residual operand exclude each other (as in LinearFn's epilogues)")
        x2 = _as_bf16_2d(x)
        wshape = weight.shape
        weight, bias = whole_param(weight), whole_param(bias)
        w16 = shadow_bf16(weight).view(wshape)
        # (the factors of a 1x1 convolution adapter arrive as [r, K, 1, 1] / [N, r, 1, 1] filters: the same matrices)
        a16, b16 = shadow_bf16(A).view(A.shape[0], -1), shadow_bf16(Bm).view(Bm.shape[0], -1)
        bias_f = None if bias is None else bias.detach().reshape(-1).contiguous()
        m, n = x2.shape[0], wshape[0]
        if residual is not None:
            r2 = _as_rows(residual)
            if not r2.is_contiguous():
                r2 = r2.contiguous()
            y = ops.gemm(x2, w16, bias=bias_f, epilogue=ops.EPI_RESIDUAL, aux_in=r2, out_dtype=r2.dtype)
        else:
            y = ops.gemm(x2, w16, bias=bias_f, out_dtype=f32 if out_f32 and act == ACT_NONE else bf16)
        ctx.p = float(p) if 0.0 < p < 1.0 else 0.0
        ctx.seed, ctx.offset = take_philox((m * n + 3) // 4) if ctx.p > 0.0 else (0, 0)
        ctx.scale = float(scale)
        h = ops.lora_down(x2, a16)
        ops.lora_up_add(y, h, b16, scale=ctx.scale, p=ctx.p, seed=ctx.seed, offset=ctx.offset)
        pre = None
        if act in (ACT_GELU, ACT_QGELU):
            pre = y
            y = ops.gelu_fwd(pre) if act == ACT_GELU else ops.quick_gelu_fwd(pre)
        ctx.save_for_backward(x2, w16, a16, b16, h, pre)
        ctx.weight, ctx.bias, ctx.A, ctx.Bm = weight, bias, A, Bm
        ctx.n = n
        ctx.has_residual = residual is not None
        ctx.x_shape = x.shape
        ctx.act = act
        return y.view(*x.shape[:-1], n)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        x2, w16, a16, b16, h, pre = ctx.saved_tensors
        weight, bias, A, Bm = ctx.weight, ctx.bias, ctx.A, ctx.Bm
        dy2 = _as_bf16_2d(dy)
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        d_res = dy2.view(*ctx.x_shape[:-1], ctx.n) if ctx.has_residual and ctx.needs_input_grad[8] else None
        if pre is not None:
            dy2 = ops.gelu_bwd(dy2, pre) if ctx.act == ACT_GELU else ops.quick_gelu_bwd(dy2, pre)
        mask = dict(p=ctx.p, seed=ctx.seed, offset=ctx.offset)
        gw = gb = ga = gbm = None
        base_owes = weight.requires_grad or (bias is not None and bias.requires_grad)
        if base_owes and _all_direct(weight, bias):  # as LinearFn: beside the dX GEMM, or in a grouped launch
            from . import fused

            if not fused.queue_linear_dw(weight, bias, dy2, x2):
                SideStream.run(lambda: _linear_param_grads(dy2, x2, weight, bias), (dy2, x2))
        # dh = s (mask . dy) Bm feeds both d lora_down.weight and the adapter's share of dx
        need_dh = ctx.needs_input_grad[0] or A.requires_grad
        dh = ops.lora_down(dy2, b16, f_trans=True, scale=ctx.scale, **mask) if need_dh else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx2 = ops.gemm(dy2, w16, b_trans=True)
            ops.lora_up_add(dx2, dh, a16, f_trans=True)
            dx = dx2.view(ctx.x_shape)  # bf16; autograd casts if needed
        if base_owes and not _all_direct(weight, bias):
            gw, gb = _linear_param_grads(dy2, x2, weight, bias)
        if Bm.requires_grad:
            gbm = param_grad(Bm, lambda out, acc: ops.lora_wgrad(dy2, h, out.view(b16.shape), accumulate=acc, scale=ctx.scale, **mask))
        if A.requires_grad:
            ga = param_grad(A, lambda out, acc: ops.lora_wgrad(x2, dh, out.view(a16.shape), out_trans=True, accumulate=acc))
        return dx, gw, gb, ga, gbm, None, None, None, d_res, None


def lora_linear(x: Tensor, weight: Tensor, bias: Optional[Tensor], A: Tensor, Bm: Tensor, scale: float, p: float = 0.0, *,
                act: int = ACT_NONE, residual: Optional[Tensor] = None, out_f32: bool = False) -> Tensor:
    return _apply(LoRALinearFn, x, weight, bias, A, Bm, scale, p, act, residual, out_f32)


def qkv_weights_adjacent(wq: Tensor, wk: Tensor, wv: Tensor) -> bool:
    """Three [D, C] parameters laid out back to back in ONE `optim.ParamArena` (registration order to_q, to_k, to_v, no bias
    in between: the reference's CrossAttention, attentions.py:505-512): their values, gradient slots and bf16 shadows are
    then each one contiguous [3 D, C] matrix."""
    ar = getattr(wq, "_cfhip_arena", None)
    if ar is None or getattr(wk, "_cfhip_arena", None) is not ar or getattr(wv, "_cfhip_arena", None) is not ar:
        return False
    if wq.dim() != 2 or wq.shape != wk.shape or wq.shape != wv.shape or not (wq.requires_grad and wk.requires_grad and wv.requires_grad):
        return False
    n = wq.numel()
    if wk.data_ptr() != wq.data_ptr() + 4 * n or wv.data_ptr() != wk.data_ptr() + 4 * n:
        return False
    sh = [getattr(w, "_cfhip_shadow", None) for w in (wq, wk, wv)]
    return all(t is not None for t in sh) and sh[1].data_ptr() == sh[0].data_ptr() + 2 * n and sh[2].data_ptr() == sh[1].data_ptr() + 2 * n


class QKVLinearFn(Function):
    """to_q(x) | to_k(x) | to_v(x) of a self-attention whose three bias-free projection weights are adjacent in the arena
    (`qkv_weights_adjacent`) as ONE GEMM against the [3 D, C] matrix they form: output [.., 3 D] packed for
    `packed_self_attention`.  Backward: one dX GEMM (instead of three + two adds of the partial input gradients) and one
    dW GEMM straight into the three adjacent gradient slots (instead of three GEMMs + three split-K reduces).  The UNet's 30
    self-attention modules: ~300 fewer launches per step."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, wq: Tensor, wk: Tensor, wv: Tensor) -> Tensor:
        x2 = _as_bf16_2d(x)
        d, c = wq.shape
        w16 = shadow_bf16(wq)
        shadow_bf16(wk)
        shadow_bf16(wv)
        w3 = torch.as_strided(w16, (3 * d, c), (c, 1))
        y = ops.gemm(x2, w3)
        ctx.save_for_backward(x2, w3)
        ctx.prm, ctx.x_shape = (wq, wk, wv), x.shape
        return y.view(*x.shape[:-1], 3 * d)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        x2, w3 = ctx.saved_tensors
        prm = ctx.prm
        d, c = prm[0].shape
        dy2 = _as_bf16_2d(dy)

        def param_grads() -> None:
            (g0, a0), (g1, a1), (g2, a2) = claims = claim_grads(prm)
            n = d * c
            together = (a0 == a1 == a2 and g1.data_ptr() == g0.data_ptr() + 4 * n
                        and g2.data_ptr() == g1.data_ptr() + 4 * n and g0.is_contiguous())
            if together:
                g3 = torch.as_strided(g0, (3 * d, c), (c, 1))
                ops.gemm(dy2, x2, a_trans=True, b_trans=True, out=g3, accumulate=a0, split_k=ops.pick_split_k(3 * d, c, x2.shape[0]))
            else:  # a gradient slot that is not the arena's (somebody replaced `.grad`), or mixed write / accumulate states
                for i, (g, acc) in enumerate(claims):
                    ops.gemm(dy2[:, i * d:(i + 1) * d], x2, a_trans=True, b_trans=True, out=g.view(d, c), accumulate=acc,
                             split_k=ops.pick_split_k(d, c, x2.shape[0]))
            commit_grads(prm)

        SideStream.run(param_grads, (dy2, x2))
        dx = ops.gemm(dy2, w3, b_trans=True).view(ctx.x_shape) if ctx.needs_input_grad[0] else None
        return dx, None, None, None


def qkv_linear(x: Tensor, wq: Tensor, wk: Tensor, wv: Tensor) -> Tensor:
    return _apply(QKVLinearFn, x, wq, wk, wv)


# ---------------------------------------------------------------------------------------------
# LayerNorm (K5)
# ---------------------------------------------------------------------------------------------


class LayerNormFn(Function):
    """Replaces nn.LayerNorm.forward (reference norms.py:88-89 via NormFactory)."""

    folds_dx_add = True  # a taped node hands the backward kernel the gradient x already has (`ctx.dx_add`, bf16, x's shape)

    @staticmethod
    def forward(ctx: Any, x: Tensor, weight: Tensor, bias: Tensor, eps: float, out_f32: bool = False) -> Tensor:
        x2 = _as_rows(x)
        gamma = weight.detach().contiguous()
        beta = bias.detach().contiguous()
        y, mean, rstd = ops.layernorm_fwd(x2, gamma, beta, eps, out_f32=bool(out_f32) and x2.dtype == f32)
        ctx.save_for_backward(x2, gamma, mean, rstd)
        ctx.weight, ctx.bias = weight, bias
        ctx.x_shape, ctx.in_dtype = x.shape, x.dtype
        _fanin_offer(ctx, x)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        x2, gamma, mean, rstd = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        dy2 = _as_bf16_2d(dy)
        gw = gb = None
        res: list = []
        dx_add = getattr(ctx, "dx_add", None)  # inside a taped node: the gradient x has already received from its other readers
        link = getattr(ctx, "link", None)
        if link is not None and link.pending is not None:  # fan-in link: the dY of the GEMM that added x back (see fanin_links)
            if dx_add is None and link.pending.shape == x2.shape:
                dx_add, link.pending = link.pending, None
            else:
                raise RuntimeError("cfhip: a fan-in link delivered a gradient the LayerNorm backward cannot take "
                                   f"({tuple(link.pending.shape)} for rows {tuple(x2.shape)})")
        if dx_add is not None:
            dx_add = dx_add.view(-1, dx_add.shape[-1])
        if _is_direct(weight) and _is_direct(bias):
            write_param_grad_pair(weight, bias, lambda ga, gb_, acc: res.append(ops.layernorm_bwd(
                dy2, x2, gamma, mean, rstd, dx_add=dx_add, dgamma=ga.view(-1), dbeta=gb_.view(-1), accumulate=acc)[0]))
            dx = res[0]  # the kernel reduced dgamma / dbeta straight into `.grad` (round 1-2: two device copies per call)
        else:
            dx, dg, db = ops.layernorm_bwd(dy2, x2, gamma, mean, rstd, dx_add=dx_add)
            if weight.requires_grad:
                gw = store_param_grad(weight, dg)
            if bias.requires_grad:
                gb = store_param_grad(bias, db)
        dx = dx.view(ctx.x_shape) if ctx.needs_input_grad[0] else None  # bf16; autograd casts if needed
        return dx, gw, gb, None, None


class LayerNorm4dFn(Function):
    """The reference's custom `LN.forward` on 4-D inputs (norms.py:30-46): per-sample mean / unbiased std over C*H*W, eps added to the
    standard deviation, per-channel affine — cfhip_layernorm4d_fwd / _bwd (csrc/norm.hip)."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], eps: float) -> Tensor:
        x2 = to_nchw(x if x.dtype == bf16 else ops.to_bf16(x.float().contiguous())).contiguous()
        w = None if weight is None else weight.detach().float().contiguous().view(-1)
        b = None if bias is None else bias.detach().float().contiguous().view(-1)
        y, mean, std = ops.layernorm4d_fwd(x2, w, b, eps)
        ctx.save_for_backward(x2, mean, std)
        ctx.w, ctx.eps, ctx.affine = w, float(eps), weight is not None
        ctx.shapes = (None if weight is None else weight.shape, None if bias is None else bias.shape)
        return y

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        x2, mean, std = ctx.saved_tensors
        dy2 = to_nchw(dy if dy.dtype == bf16 else ops.to_bf16(dy.float().contiguous())).contiguous()
        dw = db = None
        want_pg = ctx.affine and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        if want_pg:
            dw = torch.empty((x2.shape[1],), dtype=f32, device=x2.device)
            db = torch.empty_like(dw)
        dx = ops.layernorm4d_bwd(dy2, x2, ctx.w, mean, std, ctx.eps, want_dx=ctx.needs_input_grad[0], dweight=dw, dbias=db)
        if want_pg:
            dw, db = dw.view(ctx.shapes[0]), db.view(ctx.shapes[1])
        return dx, dw if ctx.affine and ctx.needs_input_grad[1] else None, db if ctx.affine and ctx.needs_input_grad[2] else None, None


def layer_norm_4d(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], eps: float) -> Tensor:
    return _apply(LayerNorm4dFn, x, weight, bias, eps)


def layer_norm(x: Tensor, weight: Tensor, bias: Tensor, eps: float, out_f32: bool = False) -> Tensor:
    """`out_f32`: an f32 input gives an f32 output — for a LayerNorm whose output is the RESIDUAL STREAM of the blocks behind it
    (nn.LayerNorm keeps its input's dtype under the reference's autocast; a bf16 copy is what a matrix product wants)."""
    if out_f32:
        return _apply(LayerNormFn, x, weight, bias, eps, True)
    return _apply(LayerNormFn, x, weight, bias, eps)


# ---------------------------------------------------------------------------------------------
# attention core (K3/K4)
# ---------------------------------------------------------------------------------------------


class PackedSelfAttentionFn(Function):
    """softmax(q k^T / sqrt(dh) [mask]) v on the packed projection output qkv [B, T, 3*D]
    (q | k | v along the last dim, head h = channels [h*64, (h+1)*64) of each third — the layout of
    reference attentions.py:214-216,180-185).  Output [B, T, D], heads already merged."""

    @staticmethod
    def forward(ctx: Any, qkv: Tensor, num_heads: int, keep_mask: Optional[Tensor], causal: bool,
                dropout_p: float = 0.0, head_dim: int = 64) -> Tensor:
        if qkv.dtype != bf16:
            qkv = ops.to_bf16(qkv.float().contiguous())
        if not qkv.is_contiguous():
            qkv = qkv.contiguous()
        d = qkv.shape[-1] // 3
        q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
        ctx.drop = _take_attn_dropout(dropout_p, qkv.shape[0], num_heads, qkv.shape[1], qkv.shape[1])
        ctx.hd = {} if head_dim == 64 else dict(head_dim=head_dim)  # (any multiple of 8 up to 192: the `_dh` kernels)
        o, lse = ops.attn_fwd(q, k, v, num_heads, mask=keep_mask, causal=causal, **ctx.hd, **ctx.drop)
        ctx.save_for_backward(qkv, o, lse, keep_mask)
        ctx.num_heads, ctx.causal = num_heads, causal
        return o

    @staticmethod
    def backward(ctx: Any, d_o: Tensor):  # type: ignore
        qkv, o, lse, keep_mask = ctx.saved_tensors
        d = qkv.shape[-1] // 3
        if d_o.dtype != bf16:
            d_o = ops.to_bf16(d_o.float())
        d_o = d_o.contiguous()
        dqkv = torch.empty_like(qkv)
        ops.attn_bwd(
            qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], o, d_o, lse, ctx.num_heads,
            dq=dqkv[..., :d], dk=dqkv[..., d:2 * d], dv=dqkv[..., 2 * d:], mask=keep_mask,
            causal=ctx.causal, **ctx.hd, **ctx.drop,
        )
        return dqkv, None, None, None, None, None


class AttentionCoreFn(Function):
    """Same computation for separately projected q [B,Tq,D], k / v [B,Tk,D] (cross attention), any head_dim that is
    a multiple of 8 up to 192 (reference attentions.py:498-569 `CrossAttention` -> sdp_attn)."""

    @staticmethod
    def forward(ctx: Any, q: Tensor, k: Tensor, v: Tensor, num_heads: int, keep_mask: Optional[Tensor],
                causal: bool, head_dim: int = 64, dropout_p: float = 0.0) -> Tensor:
        q, k, v = (t if t.dtype == bf16 else ops.to_bf16(t.float().contiguous()) for t in (q, k, v))
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()  # equal shapes -> k and v share strides
        ctx.drop = _take_attn_dropout(dropout_p, q.shape[0], num_heads, q.shape[1], k.shape[1])
        o, lse = ops.attn_fwd(q, k, v, num_heads, mask=keep_mask, causal=causal, head_dim=head_dim, **ctx.drop)
        ctx.save_for_backward(q, k, v, o, lse, keep_mask)
        ctx.num_heads, ctx.causal, ctx.head_dim = num_heads, causal, head_dim
        return o

    @staticmethod
    def backward(ctx: Any, d_o: Tensor):  # type: ignore
        q, k, v, o, lse, keep_mask = ctx.saved_tensors
        if d_o.dtype != bf16:
            d_o = ops.to_bf16(d_o.float())
        d_o = d_o.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ops.attn_bwd(q, k, v, o, d_o, lse, ctx.num_heads, dq=dq, dk=dk, dv=dv, mask=keep_mask, causal=ctx.causal,
                     head_dim=ctx.head_dim, **ctx.drop)
        return dq, dk, dv, None, None, None, None, None


class AttentionWeightsFn(Function):
    """(output, weights) for separately projected q / k / v — the reference's slow path `require_weights=True` /
    `customize_sdp` (attentions.py:256-268).  The output is the fused kernels' (scale = 1 / `scaling`: the slow path is
    the one place where the reference honours `qk_scale`); the weights f32 [B, H, Tq, Tk] are rebuilt from the saved
    log-sum-exp (`cfhip_attn_probs`); a gradient on the weights reaches q and k through `cfhip_attn_probs_bwd`.
    `dropout_p` > 0 (training, attentions.py:263-264: `F.dropout(weights)` BEFORE `_weights_callback` and the product with
    v): the output comes from the dropout forms of the fused kernels and the returned weights are the softmax times the SAME
    Philox keep-mask (`cfhip_attn_dropout_mask` of the call's (seed, offset)) / (1 - p): what multiplied v, as in the reference."""

    @staticmethod
    def forward(ctx: Any, q: Tensor, k: Tensor, v: Tensor, num_heads: int, keep_mask: Optional[Tensor], causal: bool,
                head_dim: int, scale: float, dropout_p: float = 0.0):
        q, k, v = (t if t.dtype == bf16 else ops.to_bf16(t.float().contiguous()) for t in (q, k, v))
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ctx.drop = _take_attn_dropout(dropout_p, q.shape[0], num_heads, q.shape[1], k.shape[1])
        o, lse = ops.attn_fwd(q, k, v, num_heads, mask=keep_mask, causal=causal, head_dim=head_dim, scale=scale, **ctx.drop)
        probs = ops.attn_probs(q, k, lse, num_heads, mask=keep_mask, causal=causal, head_dim=head_dim, scale=scale)
        if ctx.drop:
            probs.mul_(AttentionWeightsFn._drop_factor(ctx.drop, probs))
        ctx.save_for_backward(q, k, v, o, lse, keep_mask)
        ctx.num_heads, ctx.causal, ctx.head_dim, ctx.scale = num_heads, causal, head_dim, scale
        ctx.set_materialize_grads(False)
        return o, probs

    @staticmethod
    def _drop_factor(drop: dict, like: Tensor) -> Tensor:
        """keep-mask / (1 - p) of the call, f32 [B, H, Tq, Tk]; p is quantised to 1 / 256 by the kernels (ops.attn_dropout_p)"""
        b, h, tq, tk = like.shape
        keep = ops.attn_dropout_mask(b, h, tq, tk, drop["dropout_p"], drop["seed"], drop["offset"], device=like.device)
        return keep.to(f32).mul_(1.0 / (1.0 - ops.attn_dropout_p(drop["dropout_p"])))

    @staticmethod
    def backward(ctx: Any, d_o: Optional[Tensor], d_p: Optional[Tensor]):  # type: ignore
        q, k, v, o, lse, keep_mask = ctx.saved_tensors
        kw = dict(mask=keep_mask, causal=ctx.causal, head_dim=ctx.head_dim, scale=ctx.scale)
        dq = dk = dv = None
        if d_o is not None:
            d_o = (d_o if d_o.dtype == bf16 else ops.to_bf16(d_o.float())).contiguous()
            dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
            ops.attn_bwd(q, k, v, o, d_o, lse, ctx.num_heads, dq=dq, dk=dk, dv=dv, **kw, **ctx.drop)
        if d_p is not None:
            d_p = d_p.float().contiguous()
            if ctx.drop:  # weights = softmax * keep / (1 - p): the gradient on the softmax is the gradient on the weights times the same factor
                d_p = d_p * AttentionWeightsFn._drop_factor(ctx.drop, d_p)
            dq2, dk2 = ops.attn_probs_bwd(q, k, lse, d_p, ctx.num_heads, **kw)
            dq = dq2 if dq is None else ops.add(dq, dq2)
            dk = dk2 if dk is None else ops.add(dk, dk2)
        return dq, dk, dv, None, None, None, None, None, None


def attention_with_weights(q: Tensor, k: Tensor, v: Tensor, num_heads: int, keep_mask: Optional[Tensor] = None,
                           causal: bool = False, head_dim: int = 64, scale: Optional[float] = None, dropout_p: float = 0.0):
    return _apply(AttentionWeightsFn, q, k, v, num_heads, keep_mask, causal, head_dim,
                                    1.0 / math.sqrt(float(head_dim)) if scale is None else float(scale), float(dropout_p))


def _take_attn_dropout(dropout_p: float, b: int, num_heads: int, tq: int, tk: int) -> dict:
    """kernel arguments of one attention call with dropout on the probabilities: draws its (seed, offset) from the
    process-wide Philox stream; the backward passes get the same pair and regenerate the mask"""
    if not 0.0 < dropout_p < 1.0:
        return {}
    seed, offset = ops.PhiloxState.take(ops.attn_dropout_blocks(b, num_heads, tq, tk))
    return dict(dropout_p=float(dropout_p), seed=seed, offset=offset)


def packed_self_attention(qkv: Tensor, num_heads: int, keep_mask: Optional[Tensor] = None,
                          causal: bool = False, dropout_p: float = 0.0, head_dim: int = 64) -> Tensor:
    return _apply(PackedSelfAttentionFn, qkv, num_heads, keep_mask, causal, dropout_p, head_dim)


def attention_core(q: Tensor, k: Tensor, v: Tensor, num_heads: int, keep_mask: Optional[Tensor] = None,
                   causal: bool = False, head_dim: int = 64, dropout_p: float = 0.0) -> Tensor:
    return _apply(AttentionCoreFn, q, k, v, num_heads, keep_mask, causal, head_dim, dropout_p)


class AttentionWideFn(Function):
    """Single- or multi-head attention over heads of 192 < head_dim <= 512 channels (`ops.attn_wide_fwd`, csrc/attn_wide.hip): the
    bottleneck SpatialAttention of the KL autoencoder (reference attentions.py:330-370).  FORWARD ONLY: the first stage of latent
    diffusion is frozen and there is no wide-head backward kernel — an input that requires grad is refused here, by name, instead
    of ending in a missing gradient."""

    tapeable = False

    @staticmethod
    def forward(ctx: Any, q: Tensor, k: Tensor, v: Tensor, num_heads: int, head_dim: int) -> Tensor:
        if any(ctx.needs_input_grad[:3]):
            raise NotImplementedError(f"attention_wide: the wide head (head_dim {head_dim} > 192) is forward-only — there is no backward "
                                      "kernel for it; run it under torch.no_grad() (a frozen first stage) or detach its input")
        q, k, v = (t if t.dtype == bf16 else ops.to_bf16(t.float().contiguous()) for t in (q, k, v))
        return ops.attn_wide_fwd(q, k, v, num_heads, head_dim=head_dim, want_lse=False)[0]

    @staticmethod
    def backward(ctx: Any, d_o: Tensor):  # type: ignore
        raise NotImplementedError("attention_wide: the wide head is forward-only")


def attention_wide(q: Tensor, k: Tensor, v: Tensor, num_heads: int = 1, head_dim: Optional[int] = None) -> Tensor:
    return _apply(AttentionWideFn, q, k, v, num_heads, q.shape[-1] // num_heads if head_dim is None else head_dim)


# ---------------------------------------------------------------------------------------------
# small element-wise Functions used by the composed (non-fused) module paths
# ---------------------------------------------------------------------------------------------


class AddFn(Function):
    @staticmethod
    def forward(ctx: Any, a: Tensor, b: Tensor) -> Tensor:
        if a.dim() == 4 and (is_nhwc(a) or is_nhwc(b)):  # the residual adds of the UNet on NHWC rows (a layout mismatch: one transpose)
            a2, b2 = to_nhwc(a), to_nhwc(b)
            n, c, h, w = a2.shape
            return rows_to_nhwc(ops.add(nhwc_rows(a2), nhwc_rows(b2)), n, c, h, w)
        a2 = a if a.dtype == bf16 else ops.to_bf16(a.float().contiguous())
        b2 = b if b.dtype == bf16 else ops.to_bf16(b.float().contiguous())
        return ops.add(a2.contiguous(), b2.contiguous())

    @staticmethod
    def backward(ctx: Any, g: Tensor):  # type: ignore
        return g, g


class GeluFn(Function):
    @staticmethod
    def forward(ctx: Any, x: Tensor) -> Tensor:
        x2 = (x if x.dtype == bf16 else ops.to_bf16(x.float().contiguous())).contiguous()
        ctx.save_for_backward(x2)
        return ops.gelu_fwd(x2)

    @staticmethod
    def backward(ctx: Any, g: Tensor):  # type: ignore
        (x2,) = ctx.saved_tensors
        g2 = (g if g.dtype == bf16 else ops.to_bf16(g.float().contiguous())).contiguous()
        return ops.gelu_bwd(g2, x2)


def add(a: Tensor, b: Tensor) -> Tensor:
    return _apply(AddFn, a, b)


def gelu(x: Tensor) -> Tensor:
    return _apply(GeluFn, x)


# ---------------------------------------------------------------------------------------------
# ViT input stage (K8 as GEMM + K7 glue)
# ---------------------------------------------------------------------------------------------


class PatchTokensFn(Function):
    """VanillaPatchEmbed (stride == kernel Conv2d, reference high_level.py:172-188) + head-token
    concat + positional-encoding add (mixed_stacks/api.py:419-438,209-228) in three launches:
    im2row -> GEMM(+bias) -> assemble.  img [B,C,H,W] -> tokens bf16 [B, Np+1, D]."""

    @staticmethod
    def forward(ctx: Any, img: Tensor, conv_w: Tensor, conv_b: Optional[Tensor], head_token: Tensor,
                pos: Tensor) -> Tensor:
        b = img.shape[0]
        patch = conv_w.shape[-1]
        src = img if img.dtype in (f32, bf16) else img.float()
        rows = ops.im2row(src.contiguous(), patch)
        w16 = shadow_bf16(conv_w).view(conv_w.shape[0], -1)
        bias_f = None if conv_b is None else conv_b.detach().contiguous()
        patches = ops.gemm(rows, w16, bias=bias_f)
        x0 = ops.assemble_tokens_fwd(patches, head_token.detach().reshape(-1).contiguous(),
                                     pos.detach().reshape(-1).contiguous(), b)
        ctx.save_for_backward(rows)
        ctx.params = (conv_w, conv_b, head_token, pos)
        return x0

    @staticmethod
    def backward(ctx: Any, dx0: Tensor):  # type: ignore
        (rows,) = ctx.saved_tensors
        conv_w, conv_b, head_token, pos = ctx.params
        dx0 = (dx0 if dx0.dtype == bf16 else ops.to_bf16(dx0.float())).contiguous()
        d = dx0.shape[-1]
        direct = all(_is_direct(p) for p in (head_token, pos))
        g_head = g_pos = None
        if direct:
            # both written by one kernel: hand it the two destinations
            (dh, dp), acc = claim_grads_one_flag((head_token, pos), zero_new=True)
            dpatches = ops.assemble_tokens_bwd(dx0, dh.view(-1), dp.view(-1), acc)
            commit_grads((head_token, pos))
        else:
            g_head = torch.empty((d,), dtype=f32, device=dx0.device)
            g_pos = torch.empty((dx0.shape[1] * d,), dtype=f32, device=dx0.device)
            dpatches = ops.assemble_tokens_bwd(dx0, g_head, g_pos, False)
            g_head, g_pos = g_head.view(head_token.shape), g_pos.view(pos.shape)
        gw, gb = None, None
        n, k, m = conv_w.shape[0], rows.shape[1], rows.shape[0]
        split = ops.pick_split_k(n, k, m)
        if conv_w.requires_grad:
            def dw_into(out: Tensor, acc: bool) -> None:
                ops.gemm(dpatches, rows, a_trans=True, b_trans=True, out=out.view(n, k), accumulate=acc,
                         split_k=split)
            gw = param_grad(conv_w, dw_into)
        if conv_b is not None and conv_b.requires_grad:
            gb = param_grad(conv_b, lambda out, acc: ops.colsum(dpatches, out=out.view(-1), accumulate=acc))
        return None, gw, gb, g_head, g_pos


def patch_tokens(img: Tensor, conv_w: Tensor, conv_b: Optional[Tensor], head_token: Tensor,
                 pos: Tensor) -> Tensor:
    return _apply(PatchTokensFn, img, conv_w, conv_b, head_token, pos)


# ---------------------------------------------------------------------------------------------
# Conv2d general form (K8) = im2row + K1 GEMM; BatchNorm (K9/K10); LeakyReLU; global average pool
# ---------------------------------------------------------------------------------------------


# ---- NHWC activations (round 5) ------------------------------------------------------------------------------------------------
# The implicit-GEMM convolutions read and write NHWC ROWS ([B * H * W, C] bf16); modules exchange [B, C, H, W] tensors like the
# reference.  With `NHWC[0]` set (modules.UNetDiffuser.forward does it for the duration of a forward) a convolution hands its
# rows on as a channels_last VIEW — logical shape [B, C, H, W], strides (H W C, 1, W C, C), no copy — and every Function of the
# UNet path (GroupNorm, up-sampling, skip concatenation, residual add, the token <-> image hops of the SpatialTransformer)
# works on the rows behind such a view: the 318 NCHW <-> NHWC transposes of a 64^2 x 8 step are gone.  A Function that meets a
# layout it has no kernel for converts EXPLICITLY with the transpose kernel (`to_nchw` / `to_nhwc`) — never through
# `.contiguous()`, which would be a silent ATen copy.  CFHIP_UNET_NHWC=0 keeps the round-4 NCHW hand-over.


class _ThreadFlag:
    """`flag[0]` per thread: a forward on another thread (EMA evaluation, a second model) keeps its own setting."""

    def __init__(self) -> None:
        self._local = threading.local()

    def __getitem__(self, i: int) -> bool:
        return getattr(self._local, "value", False)

    def __setitem__(self, i: int, value: Any) -> None:
        self._local.value = bool(value)


NHWC = _ThreadFlag()
NHWC_ENABLED = os.environ.get("CFHIP_UNET_NHWC", "1") != "0"


def is_nhwc(x: Tensor) -> bool:
    if x.dim() != 4:
        return False
    b, c, h, w = x.shape
    return c > 1 and h * w > 1 and x.stride() == (h * w * c, 1, w * c, c)


def nhwc_rows(x: Tensor) -> Tensor:
    """the [B * H * W, C] rows behind a channels_last view (no copy)"""
    b, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(b * h * w, c)


def rows_to_nhwc(rows: Tensor, b: int, c: int, h: int, w: int) -> Tensor:
    """[B * H * W, C] rows as a [B, C, H, W] channels_last view (no copy)"""
    return rows.view(b, h, w, c).permute(0, 3, 1, 2)


def to_nchw(x: Tensor) -> Tensor:
    """dense NCHW of a 4-D activation: the transpose kernel for a channels_last view, `.contiguous()` otherwise (no-op when dense)"""
    if not is_nhwc(x):
        return x.contiguous()
    b, c, h, w = x.shape
    return ops.transpose_batched(nhwc_rows(x).view(b, h * w, c)).view(b, c, h, w)


def to_nhwc(x: Tensor) -> Tensor:
    """bf16 channels_last view of a 4-D activation (the transpose kernel when it arrives NCHW)"""
    if is_nhwc(x) and x.dtype == bf16:
        return x
    if x.dtype not in (bf16, f32):
        x = x.float()
    x = to_nchw(x)
    b, c, h, w = x.shape
    return rows_to_nhwc(ops.transpose_batched(x.view(b, c, h * w)).view(b * h * w, c), b, c, h, w)


def as_bf16_act(t: Tensor) -> Tensor:
    """a 4-D activation / gradient as bf16 in the layout it arrived in (NHWC rows stay NHWC rows)"""
    if t.dtype == bf16:
        return t
    t = t.float()
    if is_nhwc(t):
        b, c, h, w = t.shape
        return rows_to_nhwc(ops.to_bf16(nhwc_rows(t)), b, c, h, w)
    return ops.to_bf16(t.contiguous())


def _conv_weight_rows(weight: Tensor, kp: int) -> Tensor:
    """bf16 [Cout, Kp] view / zero-padded copy of the [Cout, Cin, kh, kw] weight (k = (c, ky, kx))."""
    cout = weight.shape[0]
    k = weight.numel() // cout
    w16 = shadow_bf16(weight).view(cout, k)
    if kp == k:
        return w16
    wp = torch.zeros((cout, kp), dtype=bf16, device=weight.device)
    wp[:, :k] = w16  # first layer only (K = Cin*kh*kw not a multiple of 8): a few KB
    return wp


# ---- which of Conv2dFn's three code paths a convolution takes ----------------------------------------------------------------------------
# implicit   3x3 / stride 1 / pad 1 with Cin % 32 == 0 (every ResBlock / up-sampling conv of the UNet) skips the im2row matrix:
#            cfhip_conv3x3_nhwc_bf16 gathers the taps inside the GEMM's K loop.  UNet 64^2 x 8 step: im2row + row2im were 38 ms of 140
#            (profiles/r01/prof_unet_summary.txt).  IMPLICIT_CONV = False: no convolution takes this route (A/B, tests).
#            A THIN HEAD — such a convolution onto a FEW channels that are not a multiple of 8 (the UNet's 3-channel head at full
#            resolution) — runs it on filters padded with zeros to THIN_HEAD_PAD output channels: the im2row route materialises the
#            [B H W, 9 Cin] matrix (189 MB at 64^2 x 8 x 320) in the forward, again for the weight gradient, and once more as the gradient
#            matrix that row2im folds back; the padded implicit convolution reads the 21 MB activation.  32, not 8: the input-gradient
#            convolution takes dY as its input and wants a multiple of 32 channels there.
# pointwise  1x1 / stride 1 with Cin % 8 == 0 (the skip connections of the UNet's residual blocks): the im2row matrix IS the NHWC copy of
#            x — one batched transpose instead of the gather kernel, kept for the weight gradient, and dX comes back through a transpose
#            instead of row2im (UNet 64^2 x 8: 38 im2row + 18 row2im launches, 3.7 ms).
# im2row     everything else: gather + GEMM; the matrix (k^2 times the input) is recomputed for the weight gradient, not kept.
# On the last two a Cout that is not a multiple of 8 (the 3-channel head of the UNet) would fall off the MFMA path onto the
# one-thread-per-output kernel (3.6 ms per launch at 64^2 x 8): the output channels are padded with zero filters to the next multiple.
IMPLICIT, POINTWISE, IM2ROW = "implicit", "pointwise", "im2row"
IMPLICIT_CONV = True
THIN_HEAD_IMPLICIT = True  # (A/B closed in round 5: profiles/r05/conv_thin_head_ab.txt)
THIN_HEAD_PAD = 32


def conv_route(cin: int, cout: int, kh: int, kw: int, stride: int, pad: int, dil: int, h: int, w: int) -> Tuple[str, int]:
    """(route, cp): the code path of Conv2dFn for this geometry and the number of output channels its kernels compute (`cout`, or
    `cout` plus zero filters).  Pure host logic."""
    geom = (kh, kw, stride, pad, dil)
    if IMPLICIT_CONV and geom == (3, 3, 1, 1, 1) and cin % 32 == 0 and h < 65536 and w < 65536:
        if cout % 8 == 0:
            return IMPLICIT, cout
        if THIN_HEAD_IMPLICIT and cout < THIN_HEAD_PAD:
            return IMPLICIT, THIN_HEAD_PAD
    return (POINTWISE if geom == (1, 1, 1, 0, 1) and cin % 8 == 0 else IM2ROW), (cout + 7) // 8 * 8


def _thin_head_ok(cin: int, cout: int, kh: int, kw: int, stride: int, pad: int, dil: int, h: int, w: int) -> bool:
    return cout % 8 != 0 and conv_route(cin, cout, kh, kw, stride, pad, dil, h, w) == (IMPLICIT, THIN_HEAD_PAD)


# ---- the filter matrices of a model's 3x3 convolutions packed in one launch at the top of its forward (round 6, late) -------------------
# Conv2dFn packs its filters into the two layouts of the implicit-GEMM kernel (forward; rotated for dX) on every call: the weights change
# every step.  For the zoo UNet that is 96 launches of 12-15 us on the critical queue.  `prepack_convs` does all of them in two launches
# (cfhip_conv3x3_pack_filters_grouped) into buffers that live with the parameters; Conv2dFn's implicit route picks its pair up with
# `pack_pre_lookup` while the scope of that forward lasts.  The buffers of a step are overwritten by the next forward's launch, i.e.
# after the backward that read them was issued on the same stream.
# Frozen filter packs (sampling): a model whose weights do not change across many forwards (the 50+ UNet calls of one `diffusion`
# sampler run) packs the FORWARD filter matrix of every packable 3x3 convolution once, on entry, into buffers of its own; while the
# context is active the model's forward uses these instead of packing (the rotated dX matrices are read by backward only).  Outside
# the context nothing changes.  The buffers reflect the weights at entry: a weight update inside the context is not seen (the fused
# Adam writes through raw pointers — no version counter to key on).
PACK_GROUPED = True  # (A/B: tools set the attribute)


class _Packs(threading.local):
    def __init__(self) -> None:
        self.packed: dict = {}  # the packs of the forward that runs on this thread: {id(weight): (forward matrix, rotated matrix or None)}
        self.frozen: dict = {}  # {id(model): such a dict} of every active `frozen_conv_packs`


_PACKS = _Packs()


def _pack_grouped(convs: Sequence[Any], rotated: bool, on_param: bool) -> dict:
    """{id(weight): (forward matrix, rotated matrix or None)} of `convs` out of one grouped launch; {} when there is nothing to pack.
    `rotated`: also the dX matrix where the implicit dX route takes it (Cout % 32 == 0).  `on_param`: into buffers that live on the
    parameter object (a deep copy of the model starts without them) instead of new ones."""
    if not PACK_GROUPED or not convs or not convs[0].weight.is_cuda:
        return {}
    items, packed = [], {}
    for conv in convs:
        w = conv.weight
        cout, cin = w.shape[0], w.shape[1]
        w16 = shadow_bf16(w).view(cout, cin, 3, 3)
        ent = getattr(w, "_cfhip_packed", None) if on_param else None
        if ent is None or ent[0].device != w16.device:
            ent = (torch.empty((cout, 9 * cin), dtype=bf16, device=w16.device),
                   torch.empty((cin, 9 * cout), dtype=bf16, device=w16.device) if rotated and cout % 32 == 0 else None)
            if on_param:
                w._cfhip_packed = ent
        items.append((w16, ent[0], False))
        if ent[1] is not None:
            items.append((w16, ent[1], True))
        packed[id(w)] = ent
    ops.conv3x3_pack_grouped(items)
    return packed


def prepack_convs(convs: Sequence[Any]) -> bool:
    """pack the filters of `convs` (modules with a [Cout, Cin, 3, 3] `weight` that reach Conv2dFn's implicit route untransformed) now"""
    _PACKS.packed = _pack_grouped(convs, rotated=True, on_param=True)
    return bool(_PACKS.packed)


def pack_pre_lookup(weight: Tensor):
    """(forward filter matrix, rotated one or None) of `weight` out of this forward's grouped launch, else None"""
    return _PACKS.packed.get(id(weight))


def pack_pre_clear() -> None:
    _PACKS.packed = {}


@contextlib.contextmanager
def frozen_conv_packs(model: Any):
    """pack the forward filter matrices of `model._packable_convs()` once (one grouped launch); yields {id(weight): (matrix,
    None)}, which `model.forward` uses instead of `prepack_convs` until the context exits"""
    packed = _pack_grouped(model._packable_convs(), rotated=False, on_param=False)
    key = id(model)
    prev = _PACKS.frozen.get(key)
    _PACKS.frozen[key] = packed
    try:
        yield packed
    finally:
        if prev is None:
            _PACKS.frozen.pop(key, None)
        else:
            _PACKS.frozen[key] = prev


def frozen_packs_of(model: Any) -> Optional[dict]:
    """the packs of an active `frozen_conv_packs(model)`, else None"""
    return _PACKS.frozen.get(id(model))


def pack_convs_of(model: Any) -> None:
    """the packs of this forward of `model` (until `pack_pre_clear`): the frozen ones when there are any, else packed now"""
    frozen = frozen_packs_of(model)
    _PACKS.packed = frozen if frozen is not None else _pack_grouped(model._packable_convs(), rotated=True, on_param=True)


# ---- the pieces the routes of Conv2dFn (and ConvTranspose2dFn) share --------------------------------------------------------------------
def _rows_in(x: Tensor, nhwc_in: bool) -> Tensor:
    """the NHWC bf16 rows [B * H * W, C] of x: the view behind a channels_last bf16 x, else one batched transpose of dense NCHW"""
    b, c, h, w = x.shape
    return nhwc_rows(x) if nhwc_in else ops.transpose_batched(x.view(b, c, h * w)).view(b * h * w, c)


def _rows_out(rows: Tensor, b: int, c: int, h: int, w: int, nhwc: bool) -> Tensor:
    """[B * H * W, Cp] rows as the [B, C, H, W] tensor the caller gets: handed on as a channels_last view when the caller takes
    that and no channel is padding, else one batched transpose to NCHW with the padded channels sliced off"""
    cp = rows.shape[1]
    if nhwc and cp == c:
        return rows_to_nhwc(rows, b, c, h, w)
    y = ops.transpose_batched(rows.view(b, h * w, cp)).view(b, cp, h, w)
    return y[:, :c].contiguous() if cp != c else y


def _pad_filters(w16: Tensor, bias_f: Optional[Tensor], cp: int) -> Tuple[Tensor, Optional[Tensor]]:
    """bf16 filters (output channels first) and their f32 bias with zero filters / zeros appended up to `cp` output channels"""
    cout = w16.shape[0]
    if cp == cout:
        return w16, bias_f
    wpad = torch.zeros((cp,) + tuple(w16.shape[1:]), dtype=bf16, device=w16.device)
    wpad[:cout] = w16
    if bias_f is not None:
        bpad = torch.zeros((cp,), dtype=f32, device=w16.device)
        bpad[:cout] = bias_f
        bias_f = bpad
    return wpad, bias_f


def _conv_wgrad_gemm(weight: Tensor, dy_rows: Tensor, rows: Tensor) -> Optional[Tensor]:
    """dW = dy_rows^T rows ([Cp, Kp], tn GEMM) for the [Cout, Cin, kh, kw] weight; padded rows / columns are dropped"""
    cout, cp = weight.shape[0], dy_rows.shape[1]
    k, (m, kp) = weight.numel() // cout, rows.shape
    split = ops.pick_split_k(cp, kp, m)
    if kp == k and cp == cout:
        return param_grad(weight, lambda out, acc: ops.gemm(dy_rows, rows, a_trans=True, b_trans=True, out=out.view(cout, k), accumulate=acc,
                                                             split_k=split))
    return store_param_grad(weight, ops.gemm(dy_rows, rows, a_trans=True, b_trans=True, out_dtype=f32, split_k=split)[:cout, :k])


def _conv_bias_grad(bias: Optional[Tensor], dy_rows: Tensor) -> Optional[Tensor]:
    if bias is None or not bias.requires_grad:
        return None
    if dy_rows.shape[1] == bias.numel():
        return param_grad(bias, lambda out, acc: ops.colsum(dy_rows, out=out.view(-1), accumulate=acc))
    return store_param_grad(bias, ops.colsum(dy_rows)[:bias.numel()])


def _implicit_forward(ctx: Any, x: Tensor, weight: Tensor, bias_f: Optional[Tensor], cp: int) -> Tensor:
    """IMPLICIT route.  Saves (x_rows, w16): the NHWC bf16 rows [B H W, Cin] of x (they serve the weight gradient; x itself is not
    kept) and the [Cp, Cin, 3, 3] bf16 filters (the weight's shadow; a thin head's zero-padded copy).  ctx.wr: the rotated filter matrix
    [Cin, 9 Cp] of the input-gradient convolution when that runs implicitly too (Cp % 32 == 0 and x wants a gradient), else None."""
    b, cin, h, w = ctx.xshape
    cout = weight.shape[0]
    x_rows = _rows_in(x, ctx.nhwc_in)
    w16, bias_f = _pad_filters(shadow_bf16(weight).view(cout, cin, 3, 3), bias_f, cp)
    pre = pack_pre_lookup(weight) if cp == cout else None  # both filter matrices out of the model's one launch (prepack_convs)
    wk = pre[0] if pre is not None else ops.conv3x3_pack_filters(w16, False)  # k = (ky, kx, c): a K-step = 32 channels of a tap
    y_rows = ops.conv3x3_nhwc(x_rows, wk, bias_f, b, h, w)
    ctx.save_for_backward(x_rows, w16)
    # The input gradient wants the filters rotated by 180 degrees with the channels swapped.  Without a grouped pack they are packed
    # HERE, on the caller's stream: the forward of the UNet is issue-bound (its queue drains faster than the host fills it), its
    # backward is bound by the queue — the pack costs nothing here and 35 us per layer there (47 launches, 1.65 ms of the 64^2 x 8
    # step: 62.4 -> 61.8 ms, profiles/r04/unet_pack_ahead_ab.txt; +1 GB of packed filters alive until backward).  The weights' current
    # bf16 shadow does not change before this step's backward has run.
    ctx.wr = None
    if cp % 32 == 0 and ctx.needs_input_grad[0]:
        ctx.wr = pre[1] if pre is not None and pre[1] is not None else ops.conv3x3_pack_filters(w16, True)
    return y_rows


def _implicit_param_grads(ctx: Any, x_rows: Tensor, w16: Tensor, dy_rows: Tensor) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    weight = ctx.weight
    b, cin, h, w = ctx.xshape
    cout, cp = weight.shape[0], w16.shape[0]
    gw = None
    if weight.requires_grad and ops.conv3x3_wgrad_ok(b, h, w):
        split = ops.pick_split_k(cp, 9 * cin, b * h * w)
        if cp == cout:
            gw = param_grad(weight, lambda out, acc: ops.conv3x3_wgrad_nhwc(dy_rows, x_rows, b, h, w, split, out=out.view(cout, cin, 3, 3),
                                                                             accumulate=acc))
        else:  # (the zero filters' rows are dropped)
            gw = store_param_grad(weight, ops.conv3x3_wgrad_nhwc(dy_rows, x_rows, b, h, w, split)[:cout])
    elif weight.requires_grad:  # back to NCHW for the im2row matrix the dW GEMM reads
        x = ops.transpose_batched(x_rows.view(b, h * w, cin)).view(b, cin, h, w)
        gw = _conv_wgrad_gemm(weight, dy_rows, ops.conv_im2row(x, 3, 3, 1, 1, 1))
    return gw, _conv_bias_grad(ctx.bias, dy_rows)


def _implicit_dx(ctx: Any, x_rows: Tensor, w16: Tensor, dy_rows: Tensor) -> Tensor:
    b, cin, h, w = ctx.xshape
    cp = dy_rows.shape[1]
    if cp % 32 == 0:  # dX = conv3x3(dY, filters rotated by 180 degrees, channels swapped): k = (ky, kx, co)
        return _rows_out(ops.conv3x3_nhwc(dy_rows, ctx.wr, None, b, h, w), b, cin, h, w, ctx.nhwc_in)
    return _im2row_dx(ctx, None, w16.reshape(cp, 9 * cin), dy_rows)  # (the filters seen as [Cp, 9 Cin])


def _pointwise_forward(ctx: Any, x: Tensor, weight: Tensor, bias_f: Optional[Tensor], cp: int) -> Tensor:
    """POINTWISE route.  Saves (rows, wp): the NHWC bf16 rows [B H W, Cin] of x, which ARE its im2row matrix, and the [Cp, Cin] bf16
    filter matrix (the weight's shadow, zero filters appended when Cp != Cout)."""
    rows = _rows_in(x, ctx.nhwc_in)
    wp, bias_f = _pad_filters(_conv_weight_rows(weight, rows.shape[1]), bias_f, cp)
    ctx.save_for_backward(rows, wp)
    return ops.gemm(rows, wp, bias=bias_f)  # [B*H*W, Cp] bf16


def _pointwise_param_grads(ctx: Any, rows: Tensor, wp: Tensor, dy_rows: Tensor) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    gw = _conv_wgrad_gemm(ctx.weight, dy_rows, rows) if ctx.weight.requires_grad else None
    return gw, _conv_bias_grad(ctx.bias, dy_rows)


def _pointwise_dx(ctx: Any, rows: Tensor, wp: Tensor, dy_rows: Tensor) -> Tensor:
    b, cin, h, w = ctx.xshape
    return _rows_out(ops.gemm(dy_rows, wp, b_trans=True), b, cin, h, w, ctx.nhwc_in)


def _im2row_forward(ctx: Any, x: Tensor, weight: Tensor, bias_f: Optional[Tensor], cp: int) -> Tensor:
    """IM2ROW route.  Saves (x, wp): x as dense NCHW (f32 or bf16, as it came; the im2row matrix is recomputed from it for the weight
    gradient) and the [Cp, Kp] bf16 filter matrix (K = Cin kh kw padded to a multiple of 8, zero filters appended when Cp != Cout)."""
    kh, kw, stride, pad, dil = ctx.geom[:5]
    if ctx.nhwc_in:  # strided / odd-shaped convolutions gather from NCHW (3 down-sampling layers per UNet): one transpose
        x = to_nchw(x)
    rows = ops.conv_im2row(x, kh, kw, stride, pad, dil, ctx.pad_hi)
    wp, bias_f = _pad_filters(_conv_weight_rows(weight, rows.shape[1]), bias_f, cp)
    ctx.save_for_backward(x, wp)
    return ops.gemm(rows, wp, bias=bias_f)  # [B*Ho*Wo, Cp] bf16


def _im2row_param_grads(ctx: Any, x: Tensor, wp: Tensor, dy_rows: Tensor) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    kh, kw, stride, pad, dil = ctx.geom[:5]
    gw = None
    if ctx.weight.requires_grad:
        gw = _conv_wgrad_gemm(ctx.weight, dy_rows, ops.conv_im2row(x, kh, kw, stride, pad, dil, ctx.pad_hi))
    return gw, _conv_bias_grad(ctx.bias, dy_rows)


def _im2row_dx(ctx: Any, x: Optional[Tensor], wp: Tensor, dy_rows: Tensor) -> Tensor:
    """GEMM + row2im (also the implicit route's dX when Cp % 32 != 0)"""
    kh, kw, stride, pad, dil = ctx.geom[:5]
    drows = ops.gemm(dy_rows, wp, b_trans=True)  # [M, Kp] bf16
    dx = ops.conv_row2im(drows, ctx.xshape, kh, kw, stride, pad, dil, ctx.pad_hi)
    return to_nhwc(dx) if ctx.nhwc_in else dx


_CONV_ROUTES = {IMPLICIT: (_implicit_forward, _implicit_param_grads, _implicit_dx),
                POINTWISE: (_pointwise_forward, _pointwise_param_grads, _pointwise_dx),
                IM2ROW: (_im2row_forward, _im2row_param_grads, _im2row_dx)}


class Conv2dFn(Function):
    """Replaces F.conv2d reached from Conv2d.forward (reference convs/basic.py:160-177), groups = 1: NCHW or channels_last in
    (f32 / bf16), bf16 out — channels_last when `NHWC[0]` asks for it and Cout % 8 == 0, else NCHW.  The geometry picks one of three
    routes (`conv_route`); each documents above what it saves.  ctx.route names it for backward."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int, pad: int, dil: int) -> Tensor:
        if x.dtype not in (bf16, f32):
            x = x.float()
        ctx.nhwc_in = is_nhwc(x) and x.dtype == bf16  # the producer handed its NHWC rows on: no transpose on the way in, dX goes back the same way
        if not ctx.nhwc_in:
            x = to_nchw(x)
        b, cin, h, w = x.shape
        cout, _, kh, kw = weight.shape
        ho, wo = ops.conv_out_hw(h, w, kh, kw, stride, pad, dil)
        bias_f = None if bias is None else bias.detach().reshape(-1).contiguous()
        ctx.weight, ctx.bias = weight, bias
        ctx.geom = (kh, kw, stride, pad, dil, ho, wo)
        ctx.pad_hi = None  # (the padding after the image where it differs from `pad`: Conv2dPadFn, IM2ROW only)
        ctx.xshape = (b, cin, h, w)
        ctx.route, cp = conv_route(cin, cout, kh, kw, stride, pad, dil, h, w)
        y_rows = _CONV_ROUTES[ctx.route][0](ctx, x, weight, bias_f, cp)
        return _rows_out(y_rows, b, cout, ho, wo, NHWC[0])

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        weight, bias = ctx.weight, ctx.bias
        b, ho, wo = ctx.xshape[0], ctx.geom[5], ctx.geom[6]
        x, wp = ctx.saved_tensors  # what they are is the route's business; every route saves its [Cp, ...] filters second
        cout, cp = weight.shape[0], wp.shape[0]  # cp: output channels incl. the zero filters
        _, param_grads, dx_of = _CONV_ROUTES[ctx.route]
        dy = as_bf16_act(dy)
        if cp != cout:
            dyp = torch.zeros((b, cp, ho * wo), dtype=bf16, device=dy.device)
            dyp[:, :cout] = to_nchw(dy).reshape(b, cout, ho * wo)
            dy = dyp
        if is_nhwc(dy):
            dy_rows = nhwc_rows(dy)  # the consumer's gradient arrives as NHWC rows: no transpose
        else:
            dy_rows = ops.transpose_batched(dy.contiguous().view(b, cp, ho * wo)).view(b * ho * wo, cp)
        if _all_direct(weight, bias):
            # nothing goes back through autograd: the weight / bias gradients run on the side stream beside dX
            SideStream.run(lambda: param_grads(ctx, x, wp, dy_rows), (dy_rows, x))
            gw = gb = None
        else:
            gw, gb = param_grads(ctx, x, wp, dy_rows)
        dx = dx_of(ctx, x, wp, dy_rows) if ctx.needs_input_grad[0] else None
        return dx, gw, gb, None, None, None


class Conv2dPadFn(Function):
    """F.pad(x, (pad, pad_hi, pad, pad_hi)) followed by F.conv2d(padding=0) without the padded copy: `pad` zero rows / columns before
    the image, `pad_hi` after it — the down-sampling of the autoencoder's encoder (reference cv/encoder/attn.py:14-28: (0, 1, 0, 1),
    3x3, stride 2).  Conv2dFn's IM2ROW route on the gather that takes both paddings (cfhip_conv_im2row_pad / _row2im_pad); the
    backward is Conv2dFn's, on this node's ctx."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int, pad: int, pad_hi: int, dil: int) -> Tensor:
        if x.dtype not in (bf16, f32):
            x = x.float()
        ctx.nhwc_in = is_nhwc(x) and x.dtype == bf16
        if not ctx.nhwc_in:
            x = to_nchw(x)
        b, cin, h, w = x.shape
        cout, _, kh, kw = weight.shape
        ho, wo = ops.conv_out_hw_pad(h, w, kh, kw, stride, pad, pad_hi, dil)
        bias_f = None if bias is None else bias.detach().reshape(-1).contiguous()
        ctx.weight, ctx.bias = weight, bias
        ctx.geom = (kh, kw, stride, pad, dil, ho, wo)
        ctx.pad_hi = pad_hi
        ctx.xshape = (b, cin, h, w)
        ctx.route = IM2ROW
        y_rows = _im2row_forward(ctx, x, weight, bias_f, (cout + 7) // 8 * 8)
        return _rows_out(y_rows, b, cout, ho, wo, NHWC[0])

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        return Conv2dFn.backward(ctx, dy)[:3] + (None, None, None, None)


class GroupedConv2dFn(Function):
    """F.conv2d with groups > 1 (reference convs/basic.py:160-177; depthwise = groups == Cin): the direct kernels of
    csrc/conv_grouped.hip — an option outside the benchmark configurations, correct and deterministic, not tuned."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int, pad: int, dil: int, groups: int) -> Tensor:
        x2 = to_nchw(as_bf16_act(x))
        w16 = shadow_bf16(weight).view(weight.shape)
        bias_f = None if bias is None else bias.detach().reshape(-1).contiguous()
        ctx.save_for_backward(x2, w16)
        ctx.weight, ctx.bias, ctx.geom = weight, bias, (stride, pad, dil, groups)
        return ops.conv2d_grouped_fwd(x2, w16, bias_f, stride, pad, dil, groups)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        x2, w16 = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        stride, pad, dil, groups = ctx.geom
        dy = to_nchw(as_bf16_act(dy))
        want_b = bias is not None and bias.requires_grad
        gw = gb = None
        if weight.requires_grad or want_b:
            direct_w, direct_b = _is_direct(weight), (want_b and _is_direct(bias))
            direct = [prm for prm, d in ((weight, direct_w), (bias, direct_b)) if d]
            claims = iter(claim_grads(direct))
            if direct_w:
                dw, acc_w = next(claims)
            else:
                dw, acc_w = torch.empty(weight.shape, dtype=f32, device=dy.device), False  # (also the scratch of a bias-only request)
                gw = dw if weight.requires_grad else None
            db, acc_b = None, False
            if direct_b:
                db, acc_b = next(claims)
            elif want_b:
                db = gb = torch.empty(bias.shape, dtype=f32, device=dy.device)
            ops.conv2d_grouped_bwd_weight(dy, x2, dw, acc_w, None if db is None else db.view(-1), acc_b, stride, pad, dil, groups)
            commit_grads(direct)
        dx = ops.conv2d_grouped_bwd_input(dy, w16, x2.shape, stride, pad, dil, groups) if ctx.needs_input_grad[0] else None
        return dx, gw, gb, None, None, None, None


class ConvTranspose2dFn(Function):
    """F.conv_transpose2d(x, wt, None, stride, padding, dilation=dilation), groups 1, output_padding 0 — what the reference's
    `Conv2d.forward(transpose=True)` reaches (convs/basic.py:160-177).  A transposed convolution IS the input-gradient map of the
    convolution with the same weight tensor read as [C_conv_out = Cin, C_conv_in = Cout, k, k], so the three products are the ones
    `Conv2dFn` already issues with the roles of forward and backward swapped:
      forward   y  = row2im(x_rows wt2)                       (Conv2dFn's dX route: GEMM (nn) + gather of the overlapping windows)
      backward  dx = im2row(dy) wt2^T   (Conv2dFn's forward), dwt2 = x_rows^T im2row(dy)   (its weight gradient, tn GEMM)
    x [B, Cin, h, w] -> bf16 [B, Cout, (h - 1) s - 2 p + d (k - 1) + 1, ...]; wt [Cin, Cout, k, k]."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, wt: Tensor, stride: int, pad: int, dil: int) -> Tensor:
        if x.dtype not in (bf16, f32):
            x = x.float()
        x = to_nchw(x)
        b, cin, h, w = x.shape
        cin_w, cout, kh, kw = wt.shape
        if cin_w != cin:
            raise ValueError(f"conv_transpose2d: input has {cin} channels, the weight expects {cin_w}")
        ho = (h - 1) * stride - 2 * pad + dil * (kh - 1) + 1
        wo = (w - 1) * stride - 2 * pad + dil * (kw - 1) + 1
        if ho <= 0 or wo <= 0:
            raise ValueError("conv_transpose2d: empty output")
        k = cout * kh * kw
        kp = (k + 7) // 8 * 8
        x_rows = ops.transpose_batched(x.view(b, cin, h * w)).view(b * h * w, cin)  # NHWC rows, bf16
        w2 = _conv_weight_rows(wt, kp)                                             # [Cin, Kp] bf16
        drows = ops.gemm(x_rows, w2, b_trans=True)                                 # [B h w, Kp]
        y = ops.conv_row2im(drows, (b, cout, ho, wo), kh, kw, stride, pad, dil)
        ctx.save_for_backward(x_rows, w2)
        ctx.wt = wt
        ctx.geom = (b, cin, h, w, cout, kh, kw, stride, pad, dil, k, kp)
        return y

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        x_rows, w2 = ctx.saved_tensors
        wt = ctx.wt
        b, cin, h, w, cout, kh, kw, stride, pad, dil, k, kp = ctx.geom
        rows = ops.conv_im2row(to_nchw(as_bf16_act(dy)), kh, kw, stride, pad, dil)  # [B h w, Kp]: the convolution's view of dy
        dx = gw = None
        if ctx.needs_input_grad[0]:
            if cin % 8 == 0:
                dx_rows = ops.gemm(rows, w2)  # [B h w, Cin]
            else:  # (output columns that are no multiple of 8 would leave the MFMA path: pad with zero filters, as Conv2dFn does)
                dx_rows = ops.gemm(rows, _pad_filters(w2, None, (cin + 7) // 8 * 8)[0])[:, :cin].contiguous()
            dx = ops.transpose_batched(dx_rows.view(b, h * w, cin)).view(b, cin, h, w)
        if wt.requires_grad:
            if cin % 8 == 0:
                g2 = ops.gemm(x_rows, rows, a_trans=True, b_trans=True, out_dtype=f32, split_k=ops.pick_split_k(cin, kp, rows.shape[0]))
            else:
                g2 = ops.gemm(x_rows, rows, a_trans=True, b_trans=True, out_dtype=f32)
            gw = g2[:, :k].reshape(wt.shape)
        return dx, gw, None, None, None


def conv_transpose2d(x: Tensor, wt: Tensor, stride: int, pad: int, dil: int = 1) -> Tensor:
    return _apply(ConvTranspose2dFn, x, wt, stride, pad, dil)


def conv2d(x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int, pad: int, dil: int = 1, groups: int = 1,
           pad_hi: Optional[int] = None) -> Tensor:
    """`pad_hi`: the zero padding after the image (bottom / right) where it differs from `pad` (top / left); groups = 1 only, always
    the im2row route (Conv2dPadFn)"""
    if pad_hi is not None and pad_hi != pad:
        if groups != 1:
            raise ValueError("conv2d: pad_hi is taken by the im2row route only (groups = 1)")
        return _apply(Conv2dPadFn, x, weight, bias, stride, pad, pad_hi, dil)
    if groups != 1:
        return _apply(GroupedConv2dFn, x, weight, bias, stride, pad, dil, groups)
    return _apply(Conv2dFn, x, weight, bias, stride, pad, dil)


# ---------------------------------------------------------------------------------------------
# The masked 7x7 convolution of the PixelCNN on its live taps (csrc/conv_masked.hip): the routing.  Not a route of Conv2dFn: only
# `pixelcnn.MaskedConv2d` asks for it (its autograd Function, `pixelcnn.MaskedConv2dFn`, lives beside the module as rnn.RecurrentFn
# does); every other convolution takes the path `conv_route` gives it.
# ---------------------------------------------------------------------------------------------

MASKED = "masked"      # the live-tap kernels
UNMASKED = "conv2d"    # Conv2dFn on the zeroed weight, whatever `conv_route` picks there
MASKED_CONV = True     # (A/B: tools set the attribute; False: every masked layer goes through Conv2dFn on the zeroed weight)


def masked_conv_route(cin: int, cout: int, k: int, stride: int, pad: int, dil: int, groups: int = 1) -> str:
    """MASKED for the geometry the live-tap kernels take — 7x7, stride 1, padding 3, dilation 1, groups 1, input and output channels
    in multiples of 32 (the input gradient runs the same kernel with the two sides swapped, and a 32-deep MFMA chunk must not straddle
    two taps) — else UNMASKED: the first layer without an embedding (Cin = 1, where the whole im2row matrix is 49 columns), other
    kernel sizes, strides, paddings.  Pure host logic."""
    ok = k == 7 and stride == 1 and pad == 3 and dil == 1 and groups == 1 and cin >= 32 and cout >= 32 and cin % 32 == 0 and cout % 32 == 0
    return MASKED if ok else UNMASKED


# ---------------------------------------------------------------------------------------------
# The direct 3x3 convolution of the ControlNet hint block (csrc/conv_direct.hip) and the bf16 SiLU between its layers.  Not a route of
# Conv2dFn: only `modules.ControlNet` asks for it, every other convolution takes the path `conv_route` gives it.
# ---------------------------------------------------------------------------------------------


DIRECT_HINT_CONV = True  # (A/B: tools set the attribute; False: the hint block's narrow layers go through Conv2dFn like any other)


def direct_conv_ok(cin: int, cout: int, k: int, stride: int, pad: int, dil: int) -> bool:
    """the layers DirectConv3x3Fn takes: 3x3, pad 1, dilation 1, stride 1 or 2, few input channels, 16 .. 96 output channels in whole
    MFMA tiles.  Pure host logic."""
    return k == 3 and pad == 1 and dil == 1 and stride in (1, 2) and 0 < cin <= 32 and cout % 16 == 0 and 0 < cout <= 96


def pad_hint_nhwc(x: Tensor) -> Tensor:
    """x [B, C, H, W] as the bf16 channels_last view DirectConv3x3Fn reads, C zero-padded to a multiple of 8 (the 3-channel hint)"""
    b, c, h, w = x.shape
    cp = (c + 7) // 8 * 8
    if cp != c:
        xp = torch.zeros((b, cp, h, w), dtype=x.dtype if x.dtype in (bf16, f32) else f32, device=x.device)
        xp[:, :c] = x
        x = xp
    return to_nhwc(x)


class DirectConv3x3Fn(Function):
    """F.conv2d(x, weight, bias, stride, padding=1) of a `direct_conv_ok` layer without the im2row matrix: forward and input gradient
    on cfhip_conv3x3_direct_bf16 (the activation is read in place as NHWC bf16, input channels zero-padded to a multiple of 8; an x
    that `pad_hint_nhwc` padded already is taken as it is); weight and bias gradient through what the IM2ROW route does (the matrix
    rebuilt with conv_im2row, `tn` GEMM, column sum).  `wp`: the forward filter operand when the caller holds one (frozen packs).
    Output: channels_last when `NHWC[0]` asks for it, else NCHW.  Saves the padded NHWC input and, when x wants a gradient, the
    input-gradient filter operand: it is packed HERE from the f32 weight, never in backward, where the optimizer step inside backward
    (optim.StepInBackward) may already be rewriting that weight once this layer's own gradient has been announced."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int, wp: Optional[Tensor] = None) -> Tensor:
        b, cx, h, w = x.shape
        cout, cin = weight.shape[0], weight.shape[1]
        cp = (cin + 7) // 8 * 8
        if tuple(weight.shape[2:]) != (3, 3) or cx not in (cin, cp) or not direct_conv_ok(cin, cout, 3, stride, 1, 1):
            raise ValueError(f"DirectConv3x3Fn: {cx} ({cin}) -> {cout} channels, stride {stride} is not a direct layer (functional.direct_conv_ok)")
        ctx.nhwc_in = is_nhwc(x) and x.dtype == bf16
        ctx.padded_in = cx != cin  # (such an input takes no gradient)
        x4 = nhwc_rows(pad_hint_nhwc(x)).view(b, h, w, cp)
        bias_f = None if bias is None else bias.detach().reshape(-1).contiguous()
        wf = weight.detach().contiguous()
        y = ops.conv3x3_direct(x4, wp if wp is not None else ops.conv3x3_direct_pack(wf, 0), bias_f, h, w, stride, 0)
        ctx.weight, ctx.bias, ctx.stride, ctx.xshape = weight, bias, stride, (b, cin, h, w)
        ctx.wr = ops.conv3x3_direct_pack(wf, 1) if ctx.needs_input_grad[0] and not ctx.padded_in else None
        ctx.save_for_backward(x4)
        ho, wo = y.shape[1], y.shape[2]
        return _rows_out(y.view(b * ho * wo, cout), b, cout, ho, wo, NHWC[0])

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        weight, bias, stride = ctx.weight, ctx.bias, ctx.stride
        (x4,) = ctx.saved_tensors
        b, cin, h, w = ctx.xshape
        cout, cp = weight.shape[0], x4.shape[3]
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        dy = as_bf16_act(dy)
        if is_nhwc(dy):
            dy_rows = nhwc_rows(dy)
        else:
            dy_rows = ops.transpose_batched(dy.contiguous().view(b, cout, ho * wo)).view(b * ho * wo, cout)

        def param_grads() -> Tuple[Optional[Tensor], Optional[Tensor]]:
            gw = None
            if weight.requires_grad:  # the IM2ROW route's weight gradient: NCHW, gather, tn GEMM
                xc = ops.transpose_batched(x4.view(b, h * w, cp)).view(b, cp, h, w)
                if cp != cin:
                    xc = xc[:, :cin].contiguous()
                gw = _conv_wgrad_gemm(weight, dy_rows, ops.conv_im2row(xc, 3, 3, stride, 1, 1))
            return gw, _conv_bias_grad(bias, dy_rows)

        if _all_direct(weight, bias):
            SideStream.run(param_grads, (dy_rows, x4))
            gw = gb = None
        else:
            gw, gb = param_grads()
        dx = None
        if ctx.wr is not None:
            dxr = ops.conv3x3_direct(dy_rows.view(b, ho, wo, cout), ctx.wr, None, h, w, stride, 1)
            dx = _rows_out(dxr.view(b * h * w, cp), b, cin, h, w, ctx.nhwc_in)
        return dx, gw, gb, None, None


def direct_conv3x3(x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int, wp: Optional[Tensor] = None) -> Tensor:
    return _apply(DirectConv3x3Fn, x, weight, bias, stride, wp)


class SiLUBf16Fn(Function):
    """nn.SiLU on a bf16 activation, in the layout it arrives in (the hint block's SiLU between plain convolutions, unet.py:443-455)"""

    @staticmethod
    def forward(ctx: Any, x: Tensor) -> Tensor:
        x = as_bf16_act(x)
        ctx.nhwc = is_nhwc(x)
        if ctx.nhwc:
            b, c, h, w = x.shape
            rows = nhwc_rows(x)
            ctx.save_for_backward(rows)
            return rows_to_nhwc(ops.silu_bf16_fwd(rows), b, c, h, w)
        x = x.contiguous()
        ctx.save_for_backward(x)
        return ops.silu_bf16_fwd(x)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        (x,) = ctx.saved_tensors
        if ctx.nhwc:
            b, c, h, w = dy.shape
            return rows_to_nhwc(ops.silu_bf16_bwd(nhwc_rows(to_nhwc(dy)), x), b, c, h, w)
        dy = as_bf16_act(dy)
        return ops.silu_bf16_bwd(to_nchw(dy) if dy.dim() == 4 else dy.contiguous(), x)


def silu_bf16(x: Tensor) -> Tensor:
    return _apply(SiLUBf16Fn, x)


class ScaleBf16Fn(Function):
    """`c * scale` of a ControlNet output (ddpm.py:419), in the layout it arrives in"""

    @staticmethod
    def forward(ctx: Any, x: Tensor, scale: float) -> Tensor:
        ctx.scale = float(scale)
        return ScaleBf16Fn._run(as_bf16_act(x), ctx.scale)

    @staticmethod
    def _run(x: Tensor, scale: float) -> Tensor:
        if is_nhwc(x):
            b, c, h, w = x.shape
            return rows_to_nhwc(ops.scale_bf16(nhwc_rows(x), scale), b, c, h, w)
        return ops.scale_bf16(x.contiguous(), scale)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        return ScaleBf16Fn._run(as_bf16_act(dy), ctx.scale), None


def scale_bf16(x: Tensor, scale: float) -> Tensor:
    return _apply(ScaleBf16Fn, x, scale)


# ---------------------------------------------------------------------------------------------
# Conv2d with a LoRA adapter: conv(x, W) + b + s * drop(up_1x1(down_kxk(x))) — the reference's LoRAConvHook in training mode
# (hijacks.py:157-166,208-266), k in (1, 3)
# ---------------------------------------------------------------------------------------------


class LoRAConv2dFn(Function):
    """One node around the base convolution: `Conv2dFn.forward` / `.backward` run on THIS node's ctx, unchanged (implicit 3x3 route,
    pointwise route, filter packs, side-stream weight gradients, nothing launched for a frozen base), on a bf16 NHWC input and with
    the NHWC hand-over switched on, so the adapter works on the rows behind the base's output and input gradient in place:
      forward   h = down(x) (ops.lora_down for 1x1, ops.lora_conv_down for 3x3), y_rows += s mask . (h Bm^T) (ops.lora_up_add)
      backward  dh = s (mask . dy) Bm (ops.lora_down, f_trans); dx_rows += down^T(dh) (ops.lora_up_add f_trans / ops.lora_conv_dx
                with `accumulate`: one read-modify-write pass over the dX the base wrote, no second gradient of x for autograd to add);
                dBm = s (mask . dy)^T h (ops.lora_wgrad), dA = ops.lora_wgrad(out_trans) / ops.lora_conv_wgrad
    An input that arrives NCHW pays one transpose each way, an output the caller wants NCHW (no NHWC hand-over) another pair.
    `scale` is a host float, the mask's (seed, offset) come from `take_philox`: no device sync, repeatable under a checkpoint."""

    tapeable = False  # a hooked layer never sits inside a taped node (modules._plain_children)

    @staticmethod
    def forward(ctx: Any, x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int, pad: int, dil: int, A: Tensor, Bm: Tensor,
                scale: float, p: float) -> Tensor:
        r, cin, k = A.shape[0], A.shape[1], A.shape[2]
        cout = weight.shape[0]
        if (k, pad) not in ((1, 0), (3, 1)) or dil != 1 or stride not in ((1,) if k == 1 else (1, 2)) or cin % 8 or cout % 8:
            raise NotImplementedError(f"LoRAConv2dFn: kernel {k} / stride {stride} / padding {pad} / dilation {dil} / channels "
                                      f"{cin} -> {cout} is outside the adapter kernels")
        ctx.x_nhwc = is_nhwc(x) and x.dtype == bf16
        xn = to_nhwc(x)
        b, _, h, w = xn.shape
        x_rows = nhwc_rows(xn)
        want_nhwc = NHWC[0]
        NHWC[0] = True
        try:
            y = Conv2dFn.forward(ctx, xn, weight, bias, stride, pad, dil)
        finally:
            NHWC[0] = want_nhwc
        yn = to_nhwc(y)  # (already the channels_last view, except for a 1 x 1 image)
        y_rows = nhwc_rows(yn)
        ho, wo = yn.shape[2], yn.shape[3]
        a16, b16 = shadow_bf16(A).view(A.shape), shadow_bf16(Bm).view(cout, r)
        hmid = ops.lora_down(x_rows, a16.view(r, cin)) if k == 1 else ops.lora_conv_down(x_rows, a16, b, h, w, stride)
        ctx.p = float(p) if 0.0 < p < 1.0 else 0.0
        ctx.seed, ctx.offset = take_philox((b * ho * wo * cout + 3) // 4) if ctx.p > 0.0 else (0, 0)
        ctx.scale = float(scale)
        ops.lora_up_add(y_rows, hmid, b16, scale=ctx.scale, p=ctx.p, seed=ctx.seed, offset=ctx.offset)
        ctx.lora = (x_rows, a16, b16, hmid)  # (x_rows is what Conv2dFn saved itself on the implicit and pointwise routes)
        ctx.A, ctx.Bm = A, Bm
        return yn if want_nhwc else to_nchw(yn)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        x_rows, a16, b16, hmid = ctx.lora
        A, Bm = ctx.A, ctx.Bm
        b, cin, h, w = ctx.xshape
        stride = ctx.geom[2]
        r, k = a16.shape[0], a16.shape[2]
        dyn = to_nhwc(as_bf16_act(dy))
        dy_rows = nhwc_rows(dyn)
        dx, gw, gb = Conv2dFn.backward(ctx, dyn)[:3]
        mask = dict(p=ctx.p, seed=ctx.seed, offset=ctx.offset)
        ga = gbm = None
        # dh = s (mask . dy) Bm feeds both d lora_down.weight and the adapter's share of dx
        need_dh = ctx.needs_input_grad[0] or A.requires_grad
        dh = ops.lora_down(dy_rows, b16, f_trans=True, scale=ctx.scale, **mask) if need_dh else None
        if ctx.needs_input_grad[0]:
            dxn = to_nhwc(as_bf16_act(dx))  # the tensor Conv2dFn.backward has just made: updated in place
            dx_rows = nhwc_rows(dxn)
            if k == 1:
                ops.lora_up_add(dx_rows, dh, a16.view(r, cin), f_trans=True)
            else:
                ops.lora_conv_dx(dh, a16, b, h, w, stride, out=dx_rows, accumulate=True)
            dx = dxn if ctx.x_nhwc else to_nchw(dxn)
        if Bm.requires_grad:
            gbm = param_grad(Bm, lambda out, acc: ops.lora_wgrad(dy_rows, hmid, out.view(b16.shape), accumulate=acc, scale=ctx.scale, **mask))
        if A.requires_grad:
            if k == 1:
                ga = param_grad(A, lambda out, acc: ops.lora_wgrad(x_rows, dh, out.view(r, cin), out_trans=True, accumulate=acc))
            else:
                ga = param_grad(A, lambda out, acc: ops.lora_conv_wgrad(dh, x_rows, out, b, h, w, stride, accumulate=acc))
        return dx, gw, gb, None, None, None, ga, gbm, None, None


def lora_conv2d(x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int, pad: int, dil: int, A: Tensor, Bm: Tensor,
                scale: float, p: float = 0.0) -> Tensor:
    return _apply(LoRAConv2dFn, x, weight, bias, stride, pad, dil, A, Bm, scale, p)


class BatchNormFn(Function):
    """Replaces nn.BatchNorm1d/2d.forward (reference norms.py:20-27,90-93) incl. the running-statistics update."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
                running_mean: Optional[Tensor], running_var: Optional[Tensor], eps: float, momentum: float,
                training: bool) -> Tensor:
        if x.dtype not in (bf16, f32):
            x = x.float()
        x = to_nchw(x)
        gamma = None if weight is None else weight.detach().contiguous()
        beta = None if bias is None else bias.detach().contiguous()
        y, mean, rstd = ops.batchnorm_fwd(x, gamma, beta, running_mean, running_var, eps, momentum, training)
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.weight, ctx.bias, ctx.training = weight, bias, training
        return y

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        x, gamma, mean, rstd = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        dy = to_nchw(as_bf16_act(dy)) if dy.dim() == 4 else (dy if dy.dtype == bf16 else ops.to_bf16(dy.float().contiguous()))
        dx, dg, db = ops.batchnorm_bwd(dy, x, gamma, mean, rstd, training=ctx.training,
                                       want_dx=ctx.needs_input_grad[0])
        gw = store_param_grad(weight, dg) if weight is not None and weight.requires_grad else None
        gb = store_param_grad(bias, db) if bias is not None and bias.requires_grad else None
        return dx, gw, gb, None, None, None, None, None


def batch_norm(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], running_mean: Optional[Tensor],
               running_var: Optional[Tensor], eps: float, momentum: float, training: bool) -> Tensor:
    return _apply(BatchNormFn, x, weight, bias, running_mean, running_var, eps, momentum, training)


class LeakyReLUFn(Function):
    """nn.LeakyReLU(slope) / nn.ReLU (slope 0) (reference activations.py:35-43)."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, slope: float) -> Tensor:
        if x.dtype != bf16:
            x = ops.to_bf16(x.float().contiguous())
        x = x.contiguous()
        ctx.save_for_backward(x)
        ctx.slope = slope
        return ops.leaky_relu_fwd(x, slope)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        (x,) = ctx.saved_tensors
        if dy.dtype != bf16:
            dy = ops.to_bf16(dy.float().contiguous())
        return ops.leaky_relu_bwd(dy.contiguous(), x, ctx.slope), None


def leaky_relu(x: Tensor, slope: float) -> Tensor:
    return _apply(LeakyReLUFn, x, slope)


class GlobalAvgPoolFn(Function):
    """nn.AdaptiveAvgPool2d((1, 1)) + squeeze (reference cv/encoder/vanilla.py:144,155-158): [B,C,H,W] -> [B,C]."""

    @staticmethod
    def forward(ctx: Any, x: Tensor) -> Tensor:
        if x.dtype != bf16:
            x = ops.to_bf16(x.float().contiguous())
        ctx.shape = tuple(x.shape)
        return ops.avgpool_fwd(x.contiguous())

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        if dy.dtype != bf16:
            dy = ops.to_bf16(dy.float().contiguous())
        return ops.avgpool_bwd(dy.contiguous(), ctx.shape)


def global_avg_pool(x: Tensor) -> Tensor:
    return _apply(GlobalAvgPoolFn, x)


class FocalLossFn(Function):
    """mean focal loss (reference losses/basic.py:170-206) on f32 logits with int64 labels."""

    @staticmethod
    def forward(ctx: Any, logits: Tensor, labels: Tensor, gamma: float, eps: float) -> Tensor:
        b = logits.shape[0]
        loss, dlogits = ops.softmax_focal(logits.float().contiguous(), labels, 1.0 / b, gamma=gamma, eps=eps)
        ctx.save_for_backward(dlogits)
        return loss[0] / b

    @staticmethod
    def backward(ctx: Any, g: Tensor):  # type: ignore
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None, None, None


def focal_loss(logits: Tensor, labels: Tensor, gamma: float = 2.0, eps: float = 1.0e-6) -> Tensor:
    return _apply(FocalLossFn, logits, labels, gamma, eps)


# ---------------------------------------------------------------------------------------------
# CLIP text tower: embedding lookup (+ positional add), row gather (EOT pooling), L2 normalisation
# ---------------------------------------------------------------------------------------------


class EmbeddingFn(Function):
    """nn.Embedding lookup (reference multimodal/clip.py:160-164,238) optionally fused with the learned positional
    add of `PositionalEncoding` (mixed_stacks/api.py:209-228): out f32 [..., D]."""

    @staticmethod
    def forward(ctx: Any, indices: Tensor, weight: Tensor, pos: Optional[Tensor], padding_idx: int) -> Tensor:
        t = indices.shape[-1]
        posd = None if pos is None else pos.detach().reshape(-1, pos.shape[-1])[:t].contiguous()
        out = ops.embedding_fwd(weight.detach().contiguous(), indices, posd, period=t if pos is not None else 0)
        ctx.save_for_backward(indices)
        ctx.weight, ctx.pos, ctx.padding_idx, ctx.t = weight, pos, padding_idx, t
        return out

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        (indices,) = ctx.saved_tensors
        weight, pos = ctx.weight, ctx.pos
        gw = gp = None
        if weight.requires_grad:
            def scatter(out: Tensor, acc: bool) -> None:
                if not acc:
                    out.zero_()
                ops.embedding_bwd(dy, indices, out, ctx.padding_idx)

            gw = param_grad(weight, scatter)
        if pos is not None and pos.requires_grad:
            d = dy.shape[-1]
            dy2 = dy if dy.dtype == bf16 else ops.to_bf16(dy.float().contiguous())
            g = ops.colsum(dy2.reshape(-1, ctx.t * d))  # sum over the batch of [B, T*D]
            gp = torch.zeros(pos.shape, dtype=f32, device=dy.device)
            gp.view(-1, d)[:ctx.t] = g.view(ctx.t, d)
        return None, gw, gp, None


def embedding(indices: Tensor, weight: Tensor, pos: Optional[Tensor] = None, padding_idx: int = -1) -> Tensor:
    return _apply(EmbeddingFn, indices, weight, pos, padding_idx)


class GatherRowsFn(Function):
    """x[arange(B), index] on the [B, T, D] f32 stream (reference multimodal/clip.py:247-249, EOT pooling)."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, index: Tensor) -> Tensor:
        b, t, d = x.shape
        x2 = x.float().contiguous().view(b * t, d) if x.dtype != f32 else x.contiguous().view(b * t, d)
        flat = torch.arange(b, device=x.device, dtype=torch.int64) * t + index.reshape(-1)
        ctx.save_for_backward(flat)
        ctx.shape = (b, t, d)
        return ops.embedding_fwd(x2, flat)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        (flat,) = ctx.saved_tensors
        b, t, d = ctx.shape
        dx = torch.zeros((b * t, d), dtype=f32, device=dy.device)
        ops.embedding_bwd(dy, flat, dx)
        return dx.view(b, t, d), None


def gather_rows(x: Tensor, index: Tensor) -> Tensor:
    return _apply(GatherRowsFn, x, index)


class L2NormalizeFn(Function):
    """cftool.array.l2_normalize (carefree-toolkit, not vendored): x / ||x||_2 over the last dim, no epsilon."""

    @staticmethod
    def forward(ctx: Any, x: Tensor) -> Tensor:
        y, inv = ops.l2norm_fwd(x.float().contiguous())
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        y, inv = ctx.saved_tensors
        return ops.l2norm_bwd(dy.float().contiguous(), y, inv)


def l2_normalize(x: Tensor) -> Tensor:
    return _apply(L2NormalizeFn, x)


# ---------------------------------------------------------------------------------------------
# UNet residual block pieces (reference convs/residual.py:86-253)
# ---------------------------------------------------------------------------------------------


class GroupNormFn(Function):
    """y = [SiLU](GroupNorm(x + add[:, :, None, None])): nn.GroupNorm (+ the time-embedding add in front and the
    nn.SiLU behind it, residual.py:226-247) in one kernel each way."""

    @staticmethod
    def forward(ctx: Any, x: Tensor, weight: Tensor, bias: Tensor, groups: int, eps: float, add: Optional[Tensor],
                silu: bool) -> Tensor:
        if x.dtype not in (bf16, f32):
            x = x.float()
        gamma, beta = weight.detach().contiguous(), bias.detach().contiguous()
        addc = None if add is None else add.detach().float().contiguous()
        ctx.weight, ctx.bias, ctx.groups, ctx.silu = weight, bias, groups, silu
        ctx.nhwc = None
        if is_nhwc(x) and x.dtype == bf16 and x.shape[1] % 8 == 0 and x.shape[1] <= 4096 and groups <= 64:
            # NHWC rows in, NHWC rows out (cfhip_groupnorm_nhwc_*): what sits between two implicit-GEMM convolutions
            b, c, h, w = x.shape
            rows = nhwc_rows(x)
            y_rows, mean, rstd = ops.groupnorm_nhwc_fwd(rows, b, gamma, beta, groups, eps, add=addc, silu=silu)
            ctx.save_for_backward(rows, gamma, beta, mean, rstd, addc)
            ctx.nhwc = (b, c, h, w)
            return rows_to_nhwc(y_rows, b, c, h, w)
        x = to_nchw(x)
        y, mean, rstd = ops.groupnorm_fwd(x, gamma, beta, groups, eps, add=addc, silu=silu)
        ctx.save_for_backward(x, gamma, beta, mean, rstd, addc)
        return y

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        x, gamma, beta, mean, rstd, addc = ctx.saved_tensors
        dy = as_bf16_act(dy)
        per_sample = gamma.dim() == 2  # one affine per sample: dgamma / dbeta stay [B, C] (ScaleShiftAffineFn reduces them)
        if ctx.nhwc is not None:
            b, c, h, w = ctx.nhwc
            dx_rows, dg, db, dadd = ops.groupnorm_nhwc_bwd(nhwc_rows(to_nhwc(dy)), x, b, gamma, beta, mean, rstd, ctx.groups, add=addc,
                                                           silu=ctx.silu)
            dx = rows_to_nhwc(dx_rows, b, c, h, w)
        else:
            dx, dg, db, dadd = ops.groupnorm_bwd(to_nchw(dy), x, gamma, beta, mean, rstd, ctx.groups, add=addc, silu=ctx.silu,
                                                 reduce=per_sample)
        gw = gb = None
        # both [B, C] partial sums reduced over B straight into `.grad` by ONE launch
        if not per_sample and _is_direct(ctx.weight) and _is_direct(ctx.bias) and dg.shape == db.shape and dg.dim() == 2:
            write_param_grad_pair(ctx.weight, ctx.bias, lambda ga, gb_, acc: ops.colreduce2_f32(dg, db, ga.view(-1), gb_.view(-1), acc))
            return (dx if ctx.needs_input_grad[0] else None), None, None, None, None, dadd, None
        grads = []
        for prm, g in ((ctx.weight, dg), (ctx.bias, db)):
            if not prm.requires_grad:
                grads.append(None)
            elif per_sample:
                grads.append(store_param_grad(prm, g))
            else:  # the [B, C] partial sums are reduced over B (straight into `.grad` when direct)
                grads.append(param_grad(prm, lambda out, acc, g=g: ops.colreduce_f32(g, out=out.view(-1), accumulate=acc)))
        gw, gb = grads
        return (dx if ctx.needs_input_grad[0] else None), gw, gb, None, None, dadd, None


def group_norm(x: Tensor, weight: Tensor, bias: Tensor, groups: int, eps: float, add: Optional[Tensor] = None,
               silu: bool = False) -> Tensor:
    """`weight` / `bias`: [C], or [B, C] for one affine per sample (see `scale_shift_affine`)."""
    return _apply(GroupNormFn, x, weight, bias, groups, eps, add, silu)


class ScaleShiftAffineFn(Function):
    """The scale-shift norm `norm(net) * (1 + scale) + shift` (reference residual.py:236-239) as GroupNorm with one affine
    per sample: gamma_eff[b, c] = gamma[c] (1 + scale[b, c]), beta_eff[b, c] = beta[c] (1 + scale[b, c]) + shift[b, c]
    (f32 [B, C]: a few hundred values; the normalisation itself stays one kernel).  The parameter gradients follow the
    package's direct-write protocol."""

    @staticmethod
    def forward(ctx: Any, weight: Tensor, bias: Tensor, scale: Tensor, shift: Tensor):  # type: ignore
        g, b_ = weight.detach().float(), bias.detach().float()
        sc = scale.detach().float()
        one_plus = sc + 1.0
        ctx.save_for_backward(g, b_, one_plus)
        ctx.weight, ctx.bias = weight, bias
        return (g[None, :] * one_plus).contiguous(), (b_[None, :] * one_plus + shift.detach().float()).contiguous()

    @staticmethod
    def backward(ctx: Any, dge: Tensor, dbe: Tensor):  # type: ignore
        g, b_, one_plus = ctx.saved_tensors
        dge, dbe = dge.float(), dbe.float()
        dgamma, dbeta = (dge * one_plus).sum(0), (dbe * one_plus).sum(0)
        gw = store_param_grad(ctx.weight, dgamma) if ctx.weight.requires_grad else None
        gb = store_param_grad(ctx.bias, dbeta) if ctx.bias.requires_grad else None
        dscale = dge * g[None, :] + dbe * b_[None, :]
        return gw, gb, dscale, dbe


def scale_shift_affine(weight: Tensor, bias: Tensor, scale: Tensor, shift: Tensor):
    return _apply(ScaleShiftAffineFn, weight, bias, scale, shift)


class SiLUF32Fn(Function):
    """nn.SiLU on the small fp32 time embedding [B, C] (residual.py:227)"""

    @staticmethod
    def forward(ctx: Any, x: Tensor) -> Tensor:
        x = x.float().contiguous()
        ctx.save_for_backward(x)
        return ops.silu_f32_fwd(x)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        (x,) = ctx.saved_tensors
        return ops.silu_f32_bwd(dy.float().contiguous(), x)


def silu_f32(x: Tensor) -> Tensor:
    return _apply(SiLUF32Fn, x)


# ---- the residual blocks' time-embedding projections, every block of a UNet forward in one launch (round 6) ------------------------------
# Each ResidualBlock computes Linear_i(SiLU(time_net)) from the same [B, K] embedding: per block a SiLU, a cast and an M = B GEMM on the
# critical queue, and in backward a cast, a GEMM, a copy, a SiLU' and autograd's add into the shared gradient (~160 launches per 64^2 x 8
# UNet step for 0.05 ms of arithmetic).  `time_proj_all` computes all of them at the top of the forward (cfhip_time_proj_fwd / _bwd); a
# block picks its own output up with `time_pre_lookup`.  The weight / bias gradients keep their path (one dW + db launch per block, on the
# side stream or in a grouped launch).
TIME_PROJ_GROUPED = True  # (A/B: tools set the attribute)


class _TimePre(threading.local):
    def __init__(self) -> None:
        self.src: Optional[Tensor] = None
        self.outs: dict = {}


_TIME_PRE = _TimePre()


class TimeProjAllFn(Function):
    """(emb, weights..., biases...) -> (Linear_i(SiLU(emb)) ..., bf16 SiLU(emb)).  Its backward is the EMBEDDING's gradient only (two
    launches when every block's dY is there, i.e. at the end of the UNet's backward); the weights' gradients are computed by each block's
    `TimeProjTapFn` when ITS dY arrives — an arena range of the in-backward optimizer must not wait for the end of the pass."""
    tapeable = False

    @staticmethod
    def forward(ctx: Any, emb: Tensor, count: int, *wb: Any):  # wb: count weights, then count biases (None allowed)
        weights = [whole_param(w) for w in wb[:count]]
        biases = [whole_param(b) for b in wb[count:]]
        w16 = [shadow_bf16(w).view(w.shape[0], -1) for w in weights]
        bias_f = [None if b is None else b.detach().reshape(-1).contiguous() for b in biases]
        emb = emb.contiguous()
        t16 = torch.empty(emb.shape, dtype=bf16, device=emb.device)
        outs = ops.time_proj_fwd(emb, w16, bias_f, t16)
        ctx.save_for_backward(emb, *w16)
        ctx.count = count
        ctx.mark_non_differentiable(t16)
        return tuple(outs) + (t16,)

    @staticmethod
    def backward(ctx: Any, *dys: Any):  # type: ignore
        emb = ctx.saved_tensors[0]
        w16 = ctx.saved_tensors[1:]
        count = ctx.count
        if not ctx.needs_input_grad[0]:
            return (None,) * (2 + 2 * count)
        dys = [None if dy is None else dy.float().contiguous() for dy in dys[:count]]
        d_emb = ops.time_proj_bwd(emb, w16, dys, [None] * count)
        return (d_emb, None) + (None,) * (2 * count)


class TimeProjTapFn(Function):
    """identity on one block's precomputed projection; in backward the block's weight / bias gradient (dW = dY^T SiLU(emb), db = colsum dY:
    on the side stream when they land straight in `.grad`) and dY handed on to `TimeProjAllFn`"""
    tapeable = False

    @staticmethod
    def forward(ctx: Any, pre: Tensor, t16: Tensor, weight: Tensor, bias: Optional[Tensor]) -> Tensor:
        ctx.weight, ctx.bias = whole_param(weight), whole_param(bias)
        ctx.save_for_backward(t16)
        return pre.view_as(pre)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        (t16,) = ctx.saved_tensors
        w, b = ctx.weight, ctx.bias
        gw = gb = None
        if w.requires_grad or (b is not None and b.requires_grad):
            dyf = dy.float().contiguous()
            if _all_direct(w, b):
                SideStream.run(lambda: _linear_param_grads(ops.to_bf16(dyf), t16, w, b), (dyf, t16))
            else:
                gw, gb = _linear_param_grads(ops.to_bf16(dyf), t16, w, b)
        return dy, None, gw, gb


def time_proj_all(time_net: Tensor, blocks: Sequence[Any]) -> bool:
    """Linear_i(SiLU(time_net)) of every block in `blocks` (modules with a plain `time_embedding` Linear) in one launch, kept for
    `time_pre_lookup` until `time_pre_clear`.  False (nothing done) when the grouped kernel does not take this input."""
    time_pre_clear()
    # (taped nodes — one autograd node per block, off by default — run each block's Functions on a tape of their own: per-block path)
    if (not TIME_PROJ_GROUPED or TAPED_NODES[0] or not blocks or getattr(_TAPE, "tape", None) is not None or not time_net.is_cuda or time_net.dtype != f32
            or time_net.dim() != 2 or time_net.shape[1] % 32 != 0 or time_net.shape[1] > 2048):
        return False
    pres: dict = {}
    for i in range(0, len(blocks), ops.TIME_PROJ_MAX):
        chunk = blocks[i:i + ops.TIME_PROJ_MAX]
        ws = [blk.time_embedding.weight for blk in chunk]
        bs = [blk.time_embedding.bias for blk in chunk]
        res = TimeProjAllFn.apply(time_net, len(chunk), *ws, *bs)
        for blk, out in zip(chunk, res[:-1]):
            pres[id(blk)] = (out, res[-1])
    _TIME_PRE.src = time_net
    _TIME_PRE.outs = pres
    return True


def time_pre_lookup(block: Any, time_net: Tensor) -> Optional[Tensor]:
    """`block.time_embedding(SiLU(time_net))` out of the grouped launch for exactly this `time_net` tensor, else None"""
    if _TIME_PRE.src is not time_net or getattr(_TAPE, "tape", None) is not None:
        return None
    hit = _TIME_PRE.outs.get(id(block))
    if hit is None:
        return None
    lin = block.time_embedding
    return TimeProjTapFn.apply(hit[0], hit[1], lin.weight, lin.bias)


def time_pre_clear() -> None:
    _TIME_PRE.src = None
    _TIME_PRE.outs = {}


class Upsample2Fn(Function):
    """F.interpolate(scale_factor=2, mode="nearest") (residual.py:147)"""

    @staticmethod
    def forward(ctx: Any, x: Tensor) -> Tensor:
        x = as_bf16_act(x)
        ctx.nhwc = is_nhwc(x) and x.shape[1] % 8 == 0
        if ctx.nhwc:
            b, c, h, w = x.shape
            return rows_to_nhwc(ops.upsample2_nhwc(nhwc_rows(x), b, h, w), b, c, 2 * h, 2 * w)
        return ops.upsample2_fwd(to_nchw(x))

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        dy = as_bf16_act(dy)
        if ctx.nhwc:
            b, c, h2, w2 = dy.shape
            return rows_to_nhwc(ops.upsample2_nhwc(nhwc_rows(to_nhwc(dy)), b, h2 // 2, w2 // 2, backward=True), b, c, h2 // 2, w2 // 2)
        return ops.upsample2_bwd(to_nchw(dy))


class AvgPool2Fn(Function):
    """nn.AvgPool2d(kernel_size=2, stride=2) (`ResDownsample(use_conv=False)`, residual.py:106)"""

    @staticmethod
    def forward(ctx: Any, x: Tensor) -> Tensor:
        x = as_bf16_act(x)
        ctx.nhwc = is_nhwc(x)  # (no NHWC pooling kernel: the zoo UNet down-samples with strided convolutions; one explicit hop each way)
        y = ops.avgpool2_fwd(to_nchw(x))
        return to_nhwc(y) if ctx.nhwc else y

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        dx = ops.avgpool2_bwd(to_nchw(as_bf16_act(dy)))
        return to_nhwc(dx) if ctx.nhwc else dx


class ReflectPad2dFn(Function):
    """nn.ReflectionPad2d (reference convs/basic.py:61-75: the `padding="reflection[N]"` form of Conv2d)"""

    @staticmethod
    def forward(ctx: Any, x: Tensor, pads: Tuple[int, int, int, int]) -> Tensor:
        if x.dtype not in (bf16, f32):
            x = x.float()
        ctx.pads = pads
        return ops.reflect_pad2d_fwd(to_nchw(x), pads)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        return ops.reflect_pad2d_bwd(to_nchw(as_bf16_act(dy)), ctx.pads), None


def reflect_pad2d(x: Tensor, pads: Any) -> Tensor:
    """`pads`: one int or (left, right, top, bottom), as nn.ReflectionPad2d takes them"""
    if isinstance(pads, int):
        pads = (pads,) * 4
    return _apply(ReflectPad2dFn, x, tuple(int(v) for v in pads))


def upsample2(x: Tensor) -> Tensor:
    return _apply(Upsample2Fn, x)


def avg_pool2(x: Tensor) -> Tensor:
    return _apply(AvgPool2Fn, x)


# ---------------------------------------------------------------------------------------------
# SpatialTransformer glue (reference mixed_stacks/api.py:766-893): GEGLU, NCHW <-> token-major
# ---------------------------------------------------------------------------------------------


class GegluFn(Function):
    """value * gelu(gate) with [value | gate] = the two halves of the last dim (reference activations.py:150-158)"""

    @staticmethod
    def forward(ctx: Any, vg: Tensor) -> Tensor:
        vg = (vg if vg.dtype == bf16 else ops.to_bf16(vg.float().contiguous())).contiguous()
        ctx.save_for_backward(vg)
        return ops.geglu_fwd(vg)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        (vg,) = ctx.saved_tensors
        dy = (dy if dy.dtype == bf16 else ops.to_bf16(dy.float().contiguous())).contiguous()
        return ops.geglu_bwd(dy, vg)


def geglu(vg: Tensor) -> Tensor:
    return _apply(GegluFn, vg)


class NchwToTokensFn(Function):
    """[B, C, H, W] -> token-major [B, H*W, C] (`permute(0, 2, 3, 1).reshape`), bf16"""

    @staticmethod
    def forward(ctx: Any, x: Tensor) -> Tensor:
        if x.dtype not in (bf16, f32):
            x = x.float()
        b, c, h, w = x.shape
        ctx.hw = (h, w)
        ctx.nhwc = is_nhwc(x) and x.dtype == bf16
        if ctx.nhwc:  # NHWC rows ARE the token-major matrix
            return nhwc_rows(x).view(b, h * w, c)
        return ops.transpose_batched(to_nchw(x).view(b, c, h * w))

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        b, t, c = dy.shape
        if ctx.nhwc:
            dy = dy if dy.dtype == bf16 else ops.to_bf16(dy.float().contiguous())
            return rows_to_nhwc(dy.contiguous().view(b * t, c), b, c, *ctx.hw)
        return ops.transpose_batched(dy.contiguous()).view(b, c, *ctx.hw)


class TokensToNchwFn(Function):
    """token-major [B, H*W, C] -> [B, C, H, W], bf16"""

    @staticmethod
    def forward(ctx: Any, x: Tensor, h: int, w: int) -> Tensor:
        if x.dtype not in (bf16, f32):
            x = x.float()
        b, t, c = x.shape
        if NHWC[0] and c % 8 == 0 and c > 1 and t > 1:  # the token-major matrix IS the image's NHWC rows: a view
            x = x if x.dtype == bf16 else ops.to_bf16(x.contiguous())
            return rows_to_nhwc(x.contiguous().view(b * t, c), b, c, h, w)
        return ops.transpose_batched(x.contiguous()).view(b, c, h, w)

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        b, c, h, w = dy.shape
        dy = as_bf16_act(dy)
        if is_nhwc(dy):
            return nhwc_rows(dy).view(b, h * w, c), None, None
        return ops.transpose_batched(dy.contiguous().view(b, c, h * w)), None, None


def nchw_to_tokens(x: Tensor) -> Tensor:
    return _apply(NchwToTokensFn, x)


def tokens_to_nchw(x: Tensor, h: int, w: int) -> Tensor:
    return _apply(TokensToNchwFn, x, h, w)


class ConcatChannelsFn(Function):
    """torch.cat([a, b], dim=1) for NCHW bf16 tensors (the UNet's skip connections, unet.py:311-316)"""

    @staticmethod
    def forward(ctx: Any, a: Tensor, b: Tensor) -> Tensor:
        ctx.nhwc = None
        if a.dim() == 4 and (is_nhwc(a) or is_nhwc(b)) and a.shape[1] > 1 and b.shape[1] > 1:
            # NHWC rows: every pixel row of the output is [a's channels | b's channels] — two strided row copies
            a, b = to_nhwc(a), to_nhwc(b)
            n, ca, h, w = a.shape
            cb = b.shape[1]
            out = torch.empty((n * h * w, ca + cb), dtype=bf16, device=a.device)
            ops.copy_strided2(nhwc_rows(a), out, ca, ca, ca + cb, nhwc_rows(b), out, cb, cb, ca + cb, n * h * w, dst_b_off=ca)
            ctx.nhwc = (n, ca, cb, h, w)
            return rows_to_nhwc(out, n, ca + cb, h, w)
        a = (a if a.dtype == bf16 else ops.to_bf16(a.float().contiguous())).contiguous()
        b = (b if b.dtype == bf16 else ops.to_bf16(b.float().contiguous())).contiguous()
        n, ca, cb = a.shape[0], a.shape[1], b.shape[1]
        inner = a.numel() // (n * ca)
        out = torch.empty((n, ca + cb, *a.shape[2:]), dtype=bf16, device=a.device)
        tot = (ca + cb) * inner
        ops.copy_strided2(a, out, ca * inner, ca * inner, tot, b, out, cb * inner, cb * inner, tot, n, dst_b_off=ca * inner)
        ctx.split = (ca, cb, inner)
        return out

    @staticmethod
    def backward(ctx: Any, dy: Tensor):  # type: ignore
        if ctx.nhwc is not None:
            n, ca, cb, h, w = ctx.nhwc
            rows = nhwc_rows(to_nhwc(as_bf16_act(dy)))
            da = torch.empty((n * h * w, ca), dtype=bf16, device=dy.device)
            db = torch.empty((n * h * w, cb), dtype=bf16, device=dy.device)
            ops.copy_strided2(rows, da, ca, ca + cb, ca, rows, db, cb, ca + cb, cb, n * h * w, src_b_off=ca)
            return rows_to_nhwc(da, n, ca, h, w), rows_to_nhwc(db, n, cb, h, w)
        ca, cb, inner = ctx.split
        dy = to_nchw(dy if dy.dtype == bf16 else ops.to_bf16(to_nchw(dy.float())))
        n = dy.shape[0]
        da = torch.empty((n, ca, *dy.shape[2:]), dtype=bf16, device=dy.device)
        db = torch.empty((n, cb, *dy.shape[2:]), dtype=bf16, device=dy.device)
        tot = (ca + cb) * inner
        ops.copy_strided2(dy, da, ca * inner, tot, ca * inner, dy, db, cb * inner, tot, cb * inner, n, src_b_off=ca * inner)
        return da, db


def concat_channels(a: Tensor, b: Tensor) -> Tensor:
    return _apply(ConcatChannelsFn, a, b)


# ---------------------------------------------------------------------------------------------
# gradient checkpointing (reference toolkit.py:2535-2647 `gradient_checkpoint`: `use_checkpoint=True` in the zoo
# `diffusion/ddpm` config wraps every ResidualBlockWithTimeEmbedding / SpatialTransformerBlock)
# ---------------------------------------------------------------------------------------------


class _CheckpointFn(Function):
    """Runs `fn` without recording in forward (nothing inside is saved for backward) and again, recording, inside
    backward; the gradients of that second run are what flows out.  The HIP Functions inside are re-entered under
    `torch.autograd.grad`: their parameter gradients are written straight into `.grad` (arena) during the inner
    backward and returned as None, so this node returns None for every parameter as well — nothing is counted twice.
    With 288 GB of HBM per GPU the default stays OFF; the switch is for the configurations that set it."""

    tapeable = False  # re-enters autograd: not inside a taped node

    @staticmethod
    def forward(ctx: Any, fn: Callable, n_inputs: int, *args: Any) -> Any:  # type: ignore
        ctx.fn = fn
        ctx.inputs = list(args[:n_inputs])
        ctx.params = list(args[n_inputs:])
        ctx.requires = [isinstance(x, Tensor) and x.requires_grad for x in ctx.inputs]
        ctx.nhwc = NHWC[0]  # the recomputation runs inside backward, after UNetDiffuser.forward has restored the flag: same hand-over
        keep_record, _PHILOX.record = _PHILOX.record, []
        try:
            with torch.no_grad():
                return fn(*ctx.inputs)
        finally:
            ctx.philox, _PHILOX.record = _PHILOX.record, keep_record

    @staticmethod
    def backward(ctx: Any, *grad_outputs: Any) -> Any:  # type: ignore
        for cb in backward_entered_callbacks:  # outer graph task: see the note at the list's definition
            cb()
        inputs = [x.detach().requires_grad_(r) if isinstance(x, Tensor) else x for x, r in zip(ctx.inputs, ctx.requires)]
        keep = NHWC[0]
        NHWC[0] = ctx.nhwc
        keep_replay, _PHILOX.replay = _PHILOX.replay, iter(ctx.philox)  # `take_philox` draws: the forward's pairs, in order
        try:
            with torch.enable_grad():
                outputs = ctx.fn(*[x.view_as(x) if isinstance(x, Tensor) else x for x in inputs])
        finally:
            NHWC[0] = keep
            _PHILOX.replay = keep_replay
        if isinstance(outputs, Tensor):
            outputs = (outputs,)
        wrt = [x for x, r in zip(inputs, ctx.requires) if r]
        wrt_params = [p for p in ctx.params if p.requires_grad]
        grads = torch.autograd.grad(outputs, wrt + wrt_params, grad_outputs, allow_unused=True)
        it = iter(grads[:len(wrt)])
        in_grads = [next(it) if r else None for r in ctx.requires]
        it = iter(grads[len(wrt):])
        p_grads = [next(it) if p.requires_grad else None for p in ctx.params]
        ctx.inputs = ctx.params = None
        return (None, None) + tuple(in_grads) + tuple(p_grads)


def gradient_checkpoint(fn: Callable, inputs: Any, params: Any, enabled: bool) -> Any:
    """Same call signature and semantics as the reference's `gradient_checkpoint(func, inputs, params, enabled)`."""
    if not enabled or not torch.is_grad_enabled():
        return fn(*inputs)
    inputs = tuple(inputs)
    return _apply(_CheckpointFn, fn, len(inputs), *(inputs + tuple(params)))


# ---------------------------------------------------------------------------------------------
# A12: dropout / DropPath as autograd Functions.  Forward draws (seed, offset) from ops.PhiloxState and remembers the
# pair; backward runs the SAME kernel on dy with the same pair (the mask is regenerated, never stored).
# ---------------------------------------------------------------------------------------------


class DropoutFn(Function):
    @staticmethod
    def forward(ctx: Any, x: Tensor, p: float, mask: Optional[Tensor]) -> Tensor:  # type: ignore
        ctx.p, ctx.mask = float(p), mask
        ctx.seed, ctx.offset = (0, 0) if mask is not None else ops.PhiloxState.take((x.numel() + 3) // 4)
        # the mask is indexed in the LOGICAL (NCHW) element order — what an injected mask and torch's own use: NHWC rows hop over
        ctx.nhwc = x.dim() == 4 and is_nhwc(x)
        y, _ = ops.dropout(to_nchw(x) if ctx.nhwc else x, ctx.p, seed=ctx.seed, offset=ctx.offset, mask=mask)
        return to_nhwc(y) if ctx.nhwc else y

    @staticmethod
    def backward(ctx: Any, dy: Tensor) -> Any:  # type: ignore
        dx, _ = ops.dropout(to_nchw(dy) if dy.dim() == 4 else dy.contiguous(), ctx.p, seed=ctx.seed, offset=ctx.offset, mask=ctx.mask)
        return (to_nhwc(dx) if ctx.nhwc else dx), None, None


def dropout(x: Tensor, p: float, training: bool, mask: Optional[Tensor] = None) -> Tensor:
    """nn.Dropout semantics (identity unless training and 0 < p < 1); `mask` (uint8, 1 = keep) injects the mask."""
    if not training or not 0.0 < p < 1.0:
        return x
    return _apply(DropoutFn, x, p, mask)


class DropPathFn(Function):
    @staticmethod
    def forward(ctx: Any, x: Tensor, keep_prob: float, mask: Tensor) -> Tensor:  # type: ignore
        ctx.keep_prob = float(keep_prob)
        ctx.save_for_backward(mask)
        return ops.drop_path(x, mask, ctx.keep_prob)

    @staticmethod
    def backward(ctx: Any, dy: Tensor) -> Any:  # type: ignore
        (mask,) = ctx.saved_tensors
        return ops.drop_path(dy.contiguous(), mask, ctx.keep_prob), None, None


def drop_path(x: Tensor, rate: float, training: bool, mask: Optional[Tensor] = None) -> Tensor:
    """reference customs.py:434-443: per-sample stochastic depth; `mask` (f32 [B] of 0 / 1) injects the sample mask."""
    if not training or not 0.0 < rate < 1.0:
        return x
    keep_prob = 1.0 - rate
    if mask is None:
        b = x.shape[0]
        seed, offset = ops.PhiloxState.take((b + 3) // 4)
        mask = ops.drop_path_mask(b, keep_prob, x.device, seed=seed, offset=offset)
    return _apply(DropPathFn, x, keep_prob, mask)


# ---------------------------------------------------------------------------------------------
# A16: tabular encoder
# ---------------------------------------------------------------------------------------------


class MLEncodeFn(Function):
    @staticmethod
    def forward(ctx: Any, x: Tensor, plan: Tensor, tables_ptr: Optional[Tensor], out_dim: int, *tables: Tensor) -> Tensor:  # type: ignore
        ctx.save_for_backward(x, plan)
        ctx.tables = tables
        return ops.ml_encode_fwd(x, plan, tables_ptr, out_dim)

    @staticmethod
    def backward(ctx: Any, dout: Tensor) -> Any:  # type: ignore
        x, plan = ctx.saved_tensors
        grads = [torch.zeros_like(t) if t.requires_grad else None for t in ctx.tables]
        ptrs = None
        if grads:
            ptrs = torch.tensor([0 if g is None else g.data_ptr() for g in grads], dtype=torch.int64).to(x.device)
        dx = ops.ml_encode_bwd(dout.float(), x, plan, ptrs, ctx.needs_input_grad[0])
        return (dx, None, None, None) + tuple(grads)
