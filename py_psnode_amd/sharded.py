"""Multi-GPU data parallelism over trajectories: one process per GPU, torch.distributed ("nccl" = RCCL over xGMI).

Trajectories never interact inside the solver (every op of my_solvers.py:66-78 is row-wise over the batch), so each
rank integrates its own contiguous slice with the single-GPU kernel and NO collective touches the data path.  The only
cross-batch coupling of the reference is that trajectory 0 decides the event steps for everybody
(neural_base.py:54,61): rank 0 builds the int32 event table from the global trajectory 0 and broadcasts it.
One all-gather of the [T, B/G, D] shards reassembles the batch "for the loss" (BASELINE.json north_star).
"""
import functools
from typing import Callable, Optional

import torch
import torch.distributed as dist


def shard_bounds(total: int, rank: int, world: int):
    """Contiguous, near-equal slice [lo, hi) of `total` trajectories for `rank`."""
    base, rem = divmod(total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def broadcast_event_table(t_local: torch.Tensor, event_t_local: Optional[torch.Tensor], group=None,
                          table_fn: Optional[Callable] = None) -> Optional[torch.Tensor]:
    """int32[T-1] event table every rank must use: computed on rank 0 (owner of global trajectory 0), broadcast.
    `event_t_local is None` must hold on all ranks or none."""
    if event_t_local is None:
        return None
    T = t_local.shape[0]
    if T < 2:
        return None
    if table_fn is None:
        from . import fused
        table_fn = fused.event_table
    tab = table_fn(t_local, event_t_local) if dist.get_rank(group) == 0 else torch.empty(T - 1, dtype=torch.int32, device=t_local.device)
    src = dist.get_global_rank(group, 0) if group is not None else 0
    dist.broadcast(tab, src=src, group=group)
    return tab


def require_equal_shards(Bl: int, device, group=None):
    """all_gather_into_tensor needs the same shard size on every rank; with unequal shards (B not a multiple of the world size)
    it hangs or fails inside RCCL.  One tiny max-reduce per gather raises a clear error on ALL ranks instead.  It runs on every
    call: a per-rank memo of the sizes already seen would let a rank whose size is a hit skip the collective while a rank whose
    size is new enters it (full batches, then a ragged last one) -- mismatched collectives across ranks, i.e. the very hang this
    check exists to prevent.  16 bytes next to a gather of megabytes, but reading the answer synchronises the host: a caller that
    has established the sizes once (a fixed global batch split evenly, as bench.py) passes check_shards=False on EVERY rank."""
    sizes = torch.tensor([Bl, -Bl], device=device)
    dist.all_reduce(sizes, op=dist.ReduceOp.MAX, group=group)
    hi, lo = int(sizes[0]), int(-sizes[1])
    if hi != lo:
        raise ValueError(f"the all-gather needs equal shards on every rank (this rank {Bl}, range {lo}..{hi} trajectories): "
                         "pad the batch or shard a multiple of the world size")


_require_equal_shards = require_equal_shards


GATHER_ALGOS = ("rccl", "direct")


class _Works:
    """The requests of one direct gather behind the `.wait()` of a c10d Work (what _pipelined / bench.py hold)."""

    def __init__(self, reqs):
        self.reqs = list(reqs)

    def wait(self):
        for r in self.reqs:
            r.wait()
        return True


def all_gather_direct(flat: torch.Tensor, shard: torch.Tensor, group=None, async_op: bool = False):
    """All-gather WITHOUT leaving the algorithm to RCCL: rank r's `shard` [R, Bl, D] lands in flat[r] (flat = [G*R, Bl, D], rank-major, as
    all_gather_into_tensor fills it) through G - 1 point-to-point pairs issued as ONE batch (`dist.batch_isend_irecv` = one
    ncclGroupStart / End): every peer's shard crosses its OWN xGMI link.  MI355X's xGMI is a point-to-point mesh (7 links x ~153 GB/s per
    GPU, no switch): a ring all-gather pushes all G - 1 shards through one link (131 MB shards at config 5: 6.0 ms, against 2.2 ms of
    integration), the direct exchange one shard per link (0.86 ms) -- and which of the two RCCL's tuner picks for a message size is not
    the caller's to steer.  SURVEY 8(e); VERDICT round 5 item 6.  Returns a waitable (async_op) or None after waiting."""
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    shard = shard.contiguous()
    R = shard.shape[0]
    if flat.shape[0] != world * R or flat.shape[1:] != shard.shape[1:] or not flat.is_contiguous():
        raise ValueError(f"all_gather_direct: flat {tuple(flat.shape)} is not the rank-major concatenation of {world} x {tuple(shard.shape)}")
    slots = flat.view(world, R, *shard.shape[1:])
    slots[rank].copy_(shard)                                   # own rows: a local copy on the compute stream
    peer = (lambda p: dist.get_global_rank(group, p)) if group is not None else (lambda p: p)
    ops = []
    for d in range(1, world):                                  # rank r talks to r + d and r - d in round d: every round is a perfect matching
        to, frm = (rank + d) % world, (rank - d) % world
        ops.append(dist.P2POp(dist.isend, shard, peer(to), group))
        ops.append(dist.P2POp(dist.irecv, slots[frm], peer(frm), group))
    work = _Works(dist.batch_isend_irecv(ops) if ops else [])
    if async_op:
        return work
    work.wait()
    return None


def _gather_into(flat, rows, group, algo, async_op):
    if algo == "direct":
        return all_gather_direct(flat, rows, group=group, async_op=async_op)
    if algo != "rccl":
        raise ValueError(f"gather algo {algo!r}: one of {GATHER_ALGOS}")
    return dist.all_gather_into_tensor(flat, rows, group=group, async_op=async_op)


def all_gather_batch(shard: torch.Tensor, group=None, check_shards: bool = True, algo: str = "rccl") -> torch.Tensor:
    """[T, Bl, D] shards (equal Bl on every rank) -> [T, G*Bl, D] view in rank order, one all_gather_into_tensor (algo "rccl") or one batch
    of point-to-point pairs (algo "direct": all_gather_direct).  The gathered storage is rank-major [G, T, Bl, D]; the result is its
    [T, G*Bl, D] rearrangement (one device copy)."""
    world = dist.get_world_size(group)
    shard = shard.contiguous()
    T, Bl, D = shard.shape
    if check_shards:
        require_equal_shards(Bl, shard.device, group)
    flat = torch.empty((world * T, Bl, D), dtype=shard.dtype, device=shard.device)   # rank-major concatenation
    _gather_into(flat, shard, group, algo, False)
    return flat.view(world, T, Bl, D).permute(1, 0, 2, 3).reshape(T, world * Bl, D)


def chunk_bounds(T: int, chunks: int):
    """Output-row boundaries b_0=0 < ... < b_C=T of `chunks` near-equal time chunks (fewer if T is small)."""
    chunks = max(1, min(chunks, T))
    return [round(c * T / chunks) for c in range(chunks + 1)]


def _pipelined(launch, T: int, Bl: int, widths, dtype, device, chunks: int, group, gather: bool, wait: bool, want_local: bool,
               check_shards: bool = True, layout: str = "chunks", algo: str = "rccl"):
    """Shared driver of the time-chunked integrate / all-gather pipeline.  `launch(s, r1, starts, outs)` integrates grid points
    s..r1-1 from the state rows `starts` (None for the first chunk) into the buffers `outs` ([r1-s, Bl, D] each).

    Every chunk writes into ITS OWN buffer: a launch stores its first row too (= the previous chunk's last row), and that row
    must not land in memory an in-flight all-gather of the previous chunk is reading (round-1 ADVICE: formal write/read race
    across streams when the chunks shared one [T,Bl,D] tensor)."""
    b = chunk_bounds(T, chunks)
    world = dist.get_world_size(group) if gather else 1
    if gather and check_shards:
        require_equal_shards(Bl, device, group)
    works, gathered, local_rows = [], [[] for _ in widths], [[] for _ in widths]
    # layout "batch": the gather of every chunk lands in ONE [T, G*Bl, D] tensor per output -- rank r's rows at [:, r*Bl:(r+1)*Bl] -- so
    # that no assemble() pass follows.  RCCL writes contiguous buffers only: c10d's list all_gather stages each chunk flat and scatters it
    # into the strided views ON THE COLLECTIVE'S STREAM, i.e. the copy assemble() made afterwards on the compute stream now rides behind
    # each chunk's gather, overlapped with the integration of the next chunk.  layout "chunks" (default) stays zero-copy: per-chunk
    # rank-major buffers.
    if gather and layout == "batch" and algo != "rccl":
        raise ValueError("layout='batch' gathers through c10d's list all_gather (RCCL's own algorithm); the direct exchange fills rank-major chunk buffers")
    full = [torch.empty((T, world * Bl, d), dtype=dtype, device=device) for d in widths] if (gather and layout == "batch") else None
    prev = None
    for c in range(len(b) - 1):
        r0, r1 = b[c], b[c + 1]
        s = max(r0 - 1, 0)                      # first grid point of this launch (= last row of the previous chunk)
        outs = [torch.empty((r1 - s, Bl, d), dtype=dtype, device=device) for d in widths]
        launch(s, r1, prev, outs)
        prev = [o[-1:] for o in outs]
        for k, o in enumerate(outs):
            rows = o[r0 - s:]                   # rows r0..r1-1 of output k (contiguous view of the chunk buffer)
            if want_local:
                local_rows[k].append(rows)
            if gather and full is not None:
                views = [full[k][r0:r1, r * Bl:(r + 1) * Bl] for r in range(world)]
                works.append(dist.all_gather(views, rows.contiguous(), group=group, async_op=True))
            elif gather:
                buf = torch.empty((world * (r1 - r0), Bl, widths[k]), dtype=dtype, device=device)
                works.append(_gather_into(buf, rows, group, algo, True))
                gathered[k].append((r0, r1, buf.view(world, r1 - r0, Bl, widths[k])))
    local = [torch.cat(r) if want_local else None for r in local_rows]
    if wait:
        for wk in works:
            wk.wait()
    if full is not None:
        gathered = full
    return local, gathered, works


def _no_segments(what: str, kw: dict):
    """A time-chunked launch restarts every chunk from the previous chunk's last row and hands the kernels one row of x: it has neither
    the dataset rows of a multiple-shooting restart nor the restart's phase inside a chunk.  `segment=` is refused, not dropped."""
    if kw.get("segment") is not None:
        raise ValueError(f"{what}: segment={kw['segment']!r} has no time-chunked form (a chunk carries neither the dataset rows x[k] nor the "
                         "phase of the restarts); integrate the shard in one launch (fused.ode_integrate / dae_integrate)")
    if kw.get("segment_parallel") is not None:      # (likewise: it spreads the segments a pipelined call cannot have)
        raise ValueError(f"{what}: segment_parallel={kw['segment_parallel']!r} needs segment=, which has no time-chunked form; integrate the "
                         "shard in one launch (fused.ode_integrate / dae_integrate)")


def integrate_ode_pipelined(method, de_layers, t, x, z, all_initial, event_idx=None, z_jump=None, chunks: int = 4, group=None,
                            local_fn: Optional[Callable] = None, gather: bool = True, wait: bool = True, want_local: bool = True,
                            check_shards: bool = True, layout: str = "chunks", algo: str = "rccl", **kw):
    """Time-chunked integrate with the all-gather of finished chunks overlapped with the integration of later ones.

    The all-gather of one [T, Bl, xd] shard set at 8 GPUs moves ~0.9 GB into every GPU -- about as long as the
    integration itself -- so it has to be hidden.  Chunk c restarts from the last row of chunk c-1 (the
    kernels read only x[0]), which is bit-identical to one long launch.  Each finished chunk is all-gathered with
    async_op=True: RCCL runs it on its own stream after the chunk's kernel, concurrently with the next chunk's kernel.
    Returns (xs_local[T,Bl,xd] or None, gathered) where `gathered` is a list of per-chunk rank-major buffers
    [(r0, r1, buf[G, r1-r0, Bl, xd])] -- the reassembled batch in time-chunk-major order (no extra copy) -- or, with
    layout="batch", the plain [T, G*Bl, xd] tensor the chunks were gathered INTO (see _pipelined).  `want_local=False`
    skips the concatenation of the local chunks (this rank's rows are in `gathered` anyway).
    """
    _no_segments("integrate_ode_pipelined", kw)
    if local_fn is None:
        from . import fused
        local_fn = fused.ode_integrate
    T, Bl, xd = t.shape[0], x.shape[1], x.shape[2]

    def launch(s, r1, starts, outs):
        x_start = x[0:1] if starts is None else starts[0]
        ev = None if event_idx is None else event_idx[s:r1 - 1]
        local_fn(method, de_layers, t[s:r1], x_start, z[s:r1], all_initial, z_jump=z_jump, event_idx=ev, out=outs[0], **kw)

    local, gathered, works = _pipelined(launch, T, Bl, [xd], x.dtype, x.device, chunks, group, gather, wait, want_local, check_shards,
                                        layout, algo)
    if not wait:
        return local[0], gathered[0], works      # caller waits (bench.py brackets the compute stream before waiting)
    return local[0], gathered[0]


def integrate_dae_pipelined(method, de_layers, ae_layers, x_init, t, z, v, i, all_initial, event_idx=None, z_jump=None, v_jump=None,
                            chunks: int = 4, group=None, local_fn: Optional[Callable] = None, gather: bool = True, wait: bool = True,
                            want_local: bool = True, check_shards: bool = True, layout: str = "chunks", algo: str = "rccl", **kw):
    """integrate_DAE (no teacher forcing) as integrate_ode_pipelined: xs AND is shards gathered chunk by chunk behind the next
    chunk's kernel.  A chunk restarts from x_init = xs[s]; the launch recomputes i0 = g(xs[s]; z[s], v[s]) itself, which is exactly
    how is[s] was produced (my_solvers.py:121 uses the un-jumped z, v of the right grid point), so the restart is bit-identical
    to one long launch -- including an event at step s, whose i0 recomputation with the jumped inputs happens inside the loop.
    Returns ((xs_local, is_local), (gathered_x, gathered_i))."""
    _no_segments("integrate_dae_pipelined", kw)
    if local_fn is None:
        from . import fused
        local_fn = fused.dae_integrate
    T, Bl = t.shape[0], t.shape[1]
    xd, idim = x_init.shape[-1], i.shape[-1]
    x_dummy = x_init.new_zeros((1, Bl, 0))          # dataset x is only read under teacher forcing

    def launch(s, r1, starts, outs):
        xi = x_init if starts is None else starts[0][0]
        ev = None if event_idx is None else event_idx[s:r1 - 1]
        local_fn(method, de_layers, ae_layers, xi, t[s:r1], x_dummy, z[s:r1], v[s:r1], i[s:r1], all_initial, z_jump=z_jump,
                 v_jump=v_jump, event_idx=ev, out=(outs[0], outs[1]), **kw)

    local, gathered, works = _pipelined(launch, T, Bl, [xd, idim], x_init.dtype, x_init.device, chunks, group, gather, wait, want_local,
                                        check_shards, layout, algo)
    if not wait:
        return tuple(local), tuple(gathered), works
    return tuple(local), tuple(gathered)


def assemble(gathered, T: int) -> torch.Tensor:
    """[T, G*Bl, xd] copy of a pipelined gather (tests / consumers that want the plain layout)."""
    G, _, Bl, xd = gathered[0][2].shape
    out = torch.empty((T, G * Bl, xd), dtype=gathered[0][2].dtype, device=gathered[0][2].device)
    for r0, r1, buf in gathered:
        out[r0:r1] = buf.permute(1, 0, 2, 3).reshape(r1 - r0, G * Bl, xd)
    return out


def integrate_ode_sharded(method, de_layers, t, x, z, all_initial, event_t=None, z_jump=None, input_true_x=False,
                          group=None, gather=True, local_fn: Optional[Callable] = None, table_fn: Optional[Callable] = None,
                          algo: str = "rccl", **kw):
    """Each rank passes ITS shard (t[T,Bl,1], x[T,Bl,xd], z[T,Bl,zd], all_initial[Bl,n], event_t/z_jump[Bl,nE,.]).
    Returns the gathered [T, G*Bl, xd] (gather=True) or the local [T,Bl,xd].  **kw goes to local_fn as it is (kernel=, act= ...)."""
    if local_fn is None:
        from . import fused
        local_fn = fused.ode_integrate
    tab = broadcast_event_table(t, event_t, group, table_fn)
    xs = local_fn(method, de_layers, t, x, z, all_initial, z_jump=z_jump, input_true_x=input_true_x, event_idx=tab, **kw)
    return all_gather_batch(xs, group, algo=algo) if gather else xs


def integrate_dae_sharded(method, de_layers, ae_layers, x_init, t, x, z, v, i, all_initial, event_t=None, z_jump=None, v_jump=None,
                          input_true_x=False, input_true_i=False, group=None, gather=True, local_fn: Optional[Callable] = None,
                          table_fn: Optional[Callable] = None, algo: str = "rccl", **kw):
    if local_fn is None:
        from . import fused
        local_fn = fused.dae_integrate
    tab = broadcast_event_table(t, event_t, group, table_fn)
    xs, is_ = local_fn(method, de_layers, ae_layers, x_init, t, x, z, v, i, all_initial, z_jump=z_jump, v_jump=v_jump,
                       input_true_x=input_true_x, input_true_i=input_true_i, event_idx=tab, **kw)
    if not gather:
        return xs, is_
    return all_gather_batch(xs, group, algo=algo), all_gather_batch(is_, group, algo=algo)


def masked_mse_sharded(pred, target, mask, col_weight=None, t0_weight: float = 0.0, global_batch: Optional[int] = None, group=None,
                       local_fn: Optional[Callable] = None, loss_func=None):
    """The scripts' masked MSE (neural_00_ODE_01_no_encode.py:353-355, neural_01_DAE_01_no_encode.py:414-419) over a batch
    that is sharded across ranks, WITHOUT gathering the predictions: two scalar-sized all-reduces instead of the
    [T,B,D] all-gather.

    Each rank passes its shard (pred/target [Bl,T,D], mask [Bl,T,1|D]).  sum(mask) is all-reduced first so that every rank
    normalises by the GLOBAL mask count; the local kernel then yields this rank's share of the global loss (and, through
    autograd, exactly the global loss's gradient w.r.t. the local predictions); the per-column terms are all-reduced for
    logging.  Returns (local_share, global_terms): call .backward() on local_share, then all_reduce_param_grads().
    t0_weight = coefficient of the mean squared error at t = 0 (`Loss_func(x[:,0,:], x_pred[:,0,:])`), normalised by the
    GLOBAL batch (global_batch, default world * Bl).
    loss_func: the scripts' `Loss_func` (loss.loss_kind_of) of the default local kernel call, loss.masked_loss; the normalisation by the
    global mask count does not depend on it.  An explicit local_fn is called as before and decides its own pointwise loss (giving both
    is a ValueError)."""
    if local_fn is not None and loss_func is not None:
        raise ValueError("masked_mse_sharded: loss_func goes to the default local call; an explicit local_fn carries its own")
    if local_fn is None:
        from . import loss
        local_fn = functools.partial(loss.masked_loss, loss_func=loss_func)
    world = dist.get_world_size(group)
    Bl, _, D = pred.shape
    msum = torch.sum(mask).reshape(1)
    dist.all_reduce(msum, group=group)
    gb = global_batch if global_batch is not None else world * Bl
    share, terms = local_fn(pred, target, mask, col_weight=col_weight, inv_norm=msum.reciprocal(), t0_coef=t0_weight / (gb * D))
    terms = terms.detach().clone()
    dist.all_reduce(terms, group=group)
    return share, terms


def all_reduce_param_grads(params, group=None):
    """Sum the parameter gradients over ranks in ONE all-reduce of a flat bucket (the ODE_01 DE_Func is 10 824 floats =
    43 KB, far below any bucketing threshold).  The sharded loss is already a share of the global loss, so the sum -- not
    the mean -- is the global gradient."""
    ps = [q for q in params if q.grad is not None]
    if not ps:
        return
    flat = torch.cat([q.grad.reshape(-1) for q in ps])
    dist.all_reduce(flat, group=group)
    off = 0
    for q in ps:
        n = q.grad.numel()
        q.grad.copy_(flat[off:off + n].view_as(q.grad))
        off += n
