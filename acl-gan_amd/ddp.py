"""Gradient averaging across ranks for data-parallel training (one process per GPU).

Not present in the reference (single GPU); new functionality for the 2/4/8-GPU
rows of BASELINE.json.  All normalisation layers on the path are per-sample (IN / AdaIN / custom
LN), the LSGAN / L1 losses are batch means, so averaging per-rank gradients of a batch shard is
exactly the large-batch gradient -- except for the focus 'size' loss, which squares a sum over
the *local* batch (trainer.py:149-150); per-rank evaluation + averaging is standard DDP
semantics and is what this module implements (documented in DESIGN.md).

The flat gradient buffer of one optimizer (120 MB gen / 99 MB dis in fp32) is reduced in a few
large buckets: xGMI is point-to-point (7 links x ~153 GB/s per GPU), large messages keep RCCL on
its bandwidth-optimal algorithms, and the step is O(100 ms) so latency is irrelevant.
"""
import ctypes
import os
import warnings

import torch
import torch.distributed as dist

from . import _lib as L

BUCKET_ELEMS = 16 * 1024 * 1024   # 64 MB fp32 per collective (post-backward path)
# overlapped path: smaller buckets become ready earlier.  4 M floats = 16 MB: still far above the size where an
# xGMI all-reduce is latency-bound (each GPU pushes 1/8 of a bucket to each of its 7 peers over its own link).
OVERLAP_BUCKET_ELEMS = int(os.environ.get("ACLGAN_DDP_BUCKET_ELEMS", 4 * 1024 * 1024))


def allreduce_flat(flat: torch.Tensor, world_size: int, bucket_elems: int = BUCKET_ELEMS):
    """In-place average of ``flat`` over all ranks."""
    backend = dist.get_backend()
    use_avg = backend == "nccl"   # RCCL implements ReduceOp.AVG; gloo (CPU tests) does not
    works = []
    n = flat.numel()
    for s in range(0, n, bucket_elems):
        chunk = flat[s: min(n, s + bucket_elems)]
        works.append(dist.all_reduce(chunk, op=dist.ReduceOp.AVG if use_avg else dist.ReduceOp.SUM, async_op=True))
    for w in works:
        w.wait()
    if not use_avg:
        flat.mul_(1.0 / world_size)
    return flat


def shard_batch(x: torch.Tensor, rank: int, world_size: int) -> torch.Tensor:
    """rank r gets samples [r*b, (r+1)*b) of a global batch."""
    b = x.shape[0] // world_size
    assert b * world_size == x.shape[0], "global batch must divide by world size"
    return x[rank * b: (rank + 1) * b]


def broadcast_flat(flat: torch.Tensor, src: int = 0, bucket_elems: int = BUCKET_ELEMS):
    """Overwrite ``flat`` on every rank with rank ``src``'s copy (replica initialisation)."""
    n = flat.numel()
    works = [dist.broadcast(flat[s: min(n, s + bucket_elems)], src, async_op=True) for s in range(0, n, bucket_elems)]
    for w in works:
        w.wait()
    return flat


class BucketReducer:
    """Gradient all-reduce overlapped with the backward pass.

    The engine (csrc/engine.hip::run_tape) knows, for the static graph of an update, which backward closure is the last
    writer of every bucket of the trained group's flat gradient buffer, and calls back on the host right after that
    closure's kernels have been enqueued.  The callback starts ``dist.all_reduce(bucket, async_op=True)``:
    ProcessGroupNCCL orders the collective (on its own RCCL stream) after everything enqueued on the compute stream so
    far and nothing enqueued later waits for it, so the exchange runs concurrently with the remaining dgrad / wgrad
    kernels.  ``finish()`` makes the compute stream wait for all of them; Adam follows.  Completion order is a function
    of the graph only, hence identical on all ranks (collectives match up).

    ctx: the aclgan_ctx handle; grad_of(group) -> that group's flat gradient tensor."""

    def __init__(self, ctx, grad_of, world_size: int, bucket_elems: int = OVERLAP_BUCKET_ELEMS):
        self.ctx, self.grad_of, self.world = ctx, grad_of, world_size
        self.bucket_elems = int(bucket_elems)
        self.use_avg = dist.get_backend() == "nccl"   # RCCL has ReduceOp.AVG; gloo (CPU tests) sums, then scales
        self.works, self.order, self.error, self.group = [], [], None, None
        self._cb = L.BUCKET_FN(self._on_bucket)       # must outlive the registration
        L.check(L.lib.aclgan_set_grad_buckets(ctx, self.bucket_elems, self._cb, None), "set_grad_buckets")

    def close(self):
        L.lib.aclgan_set_grad_buckets(self.ctx, 0, ctypes.cast(None, L.BUCKET_FN), None)

    def begin(self, group: int):
        self.works, self.order, self.error, self.group = [], [], None, group

    def _on_bucket(self, user, group, bucket, offset, numel):
        try:   # an exception must not unwind through the C frames of the engine
            chunk = self.grad_of(group)[offset: offset + numel]
            op = dist.ReduceOp.AVG if self.use_avg else dist.ReduceOp.SUM
            self.works.append((dist.all_reduce(chunk, op=op, async_op=True), chunk))
            self.order.append(int(bucket))
        except BaseException as e:   # noqa: BLE001
            self.error = e

    def finish(self, group: int):
        if self.error is not None:
            raise self.error
        n = self.grad_of(group).numel()
        want = (n + self.bucket_elems - 1) // self.bucket_elems
        if len(self.works) != want or sorted(self.order) != list(range(want)):
            raise RuntimeError("bucket reducer: %d of %d buckets of group %d were reduced (%s)" % (len(self.works), want, group, self.order))
        for w, chunk in self.works:
            w.wait()
            if not self.use_avg:
                chunk.mul_(1.0 / self.world)
        self.works = []


class DataParallel:
    """The data-parallel side of aclgan_Trainer, a base class of it (not in the reference): one process per GPU, full replicas"""

    def _dist_world(self):
        if not (dist.is_available() and dist.is_initialized()):
            return 0
        if dist.get_world_size() == 1 and os.environ.get("ACLGAN_BENCH_FORCE_DIST") != "1":
            return 0
        return dist.get_world_size()

    def _setup_data_parallel(self):
        """Called at the end of __init__ and resume(): replicas must START identical, whatever each rank's RNG did -- broadcast rank 0's
        state; then hook the engine's bucket callback so that each gradient bucket's all-reduce starts while the rest of the backward is
        still running (BucketReducer).
        z noise: every rank draws its own shard's z from a generator seeded with initial_seed() + rank."""
        self._reducer = None
        self._exposed_events, self._exposed_ms = [], 0.0
        world = self._dist_world()
        if not world:
            return
        # parameters and Adam state; the average; spectral norm's u / v (not parameters); the LeCam anchors and ADA's p and counters -- which
        # every rank then keeps for itself: each sees its own shard, neither is all-reduced (the ranks may drift apart in p)
        start = [buf for grp in (L.GROUP_GEN, L.GROUP_DIS) for buf in (self._param[grp], self._m[grp], self._v[grp])]
        start += [self._ema, self._sn_state if self._tensors[L.GROUP_SN_STATE] else None, self._lecam, self._ada]
        for buf in (b for b in start if b is not None):
            broadcast_flat(buf)
        steps = torch.tensor([self._opt[0]["steps"], self._opt[1]["steps"], self._sched_calls], dtype=torch.int64, device=self.device)
        dist.broadcast(steps, 0)
        self._opt[0]["steps"], self._opt[1]["steps"], self._sched_calls = (int(v) for v in steps.tolist())
        self._zgen = torch.Generator().manual_seed(torch.initial_seed() + dist.get_rank())
        if os.environ.get("ACLGAN_DDP_OVERLAP", "1") != "0":
            self._reducer = BucketReducer(self._ctx, lambda g: self._grad[g], world)
        if self.hip_graph:
            # HIP-graph replay is single-GPU only: the bucket callbacks and the forward sync point are host code that starts
            # collectives from inside the update, which a captured graph cannot replay -- say so instead of silently ignoring the option
            warnings.warn("aclgan_Trainer: hip_graph=True is ignored in data-parallel runs (world size %d): updates run eagerly" % world)
            self.hip_graph = False
        # optional: the reference's global-batch semantics of the focus losses (config key ddp_global_focus / env
        # ACLGAN_DDP_GLOBAL_FOCUS=1): the 6 mask sums are all-reduced at a forward sync point of gen_update
        if self._hp.get("ddp_global_focus", False) or os.environ.get("ACLGAN_DDP_GLOBAL_FOCUS") == "1":
            def on_sync(user, ptr, n):
                try:
                    off = int(ptr) - self._ws.data_ptr()
                    t = self._ws[off: off + 4 * n].view(torch.float32)
                    dist.all_reduce(t, op=dist.ReduceOp.SUM)      # stream-ordered: the compute stream waits for it, the host does not
                except BaseException as e:   # noqa: BLE001  (must not unwind through the C frames)
                    self._sync_error = e
            self._sync_error = None
            self._sync_cb = L.SYNC_FN(on_sync)
            L.check(L.lib.aclgan_set_forward_sync(self._ctx, self._sync_cb, None, world), "set_forward_sync")

    def _allreduce_grads(self, grp):
        """Average the flat gradient buffer over ranks with RCCL before Adam.  With the bucket reducer the collectives
        were started from inside the backward (overlap) and are only waited for here; ACLGAN_DDP_OVERLAP=0 selects the
        plain post-backward bucketed all-reduce.  No-op when torch.distributed is not initialised."""
        world = self._dist_world()
        if not world:
            return
        # GPU-side exposure of the exchange: the compute stream does nothing between these two events except wait for the
        # collectives, so their distance is the part of the all-reduce that was NOT hidden behind the backward
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        if self._reducer is not None:
            self._reducer.finish(grp)
        else:
            allreduce_flat(self._grad[grp], world)
        ev[1].record()
        self._exposed_events.append(ev)
        if len(self._exposed_events) > 4096:
            self.allreduce_exposed_ms()

    def allreduce_exposed_ms(self, reset=True):
        """total milliseconds the compute stream spent waiting for gradient collectives since the last call (synchronises)"""
        torch.cuda.synchronize(self.device)
        self._exposed_ms += sum(a.elapsed_time(b) for a, b in self._exposed_events)
        self._exposed_events = []
        v = self._exposed_ms
        if reset:
            self._exposed_ms = 0.0
        return v
