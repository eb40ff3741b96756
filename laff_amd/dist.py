"""Multi-GPU decomposition of the hot path (one process per GPU, torch.distributed; backend 'nccl' is RCCL over xGMI).

The reference has no parallelism of any kind; the path shards by rows and admits two
decompositions, both implemented:

  'video' (evaluate_sharded; the scheme BASELINE.json names): rank g owns videos [v0, v1) end to end (features -> embeddings ->
      its column block S[:, v0:v1]); text rows are split the same way for the embedding stage only, then ONE all-gather of the
      fp32 TEXT embeddings (Nt x K) gives every rank all texts -- issued asynchronously, it overlaps the video tower; every rank
      packs the gathered rows into the GEMM operand itself.  Ranks: the exact ground-truth score s_gt64[t] comes from the rank
      that owns gt(t) -> all-reduce(MAX) of Nt doubles; every rank counts the better-scoring videos of its block (error-band
      count + exact re-score, ops.rank_prepare / sim_gemm_banded / rank_resolve) -> all-reduce(SUM) of Nt int32.
  'text' (evaluate_sharded_by_text): rank g owns texts [t0, t1) end to end and the ROW block S[t0:t1, :]; ONE all-gather of the fp32
      VIDEO embeddings (Nv x K); every text meets its ground-truth video locally, so both all-reduces disappear; the ranks (Nt
      int32) are all-gathered for the replicated metrics.

  'video16' (evaluate_sharded_v16): the 'video' decomposition with HALF the gathered bytes on the text side -- what crosses the links is
      the 16-bit text OPERAND (Nt x K x 2 B) and the fp32 VIDEO embeddings (Nv x K x 4 B, the smaller side); the fp32 text rows never
      leave their owner.  The owner of a text scores it exactly against its ground-truth video (all fp32 video rows are there) and
      all-gathers {s_gt64, band_t} (12 B per text); every rank runs the banded GEMM of all texts x its videos; the pairs inside the
      band (8 B each) go by all-to-all to the owner of their text row, which re-scores them exactly; counts are all-reduced, ranks
      all-gathered.  No MAX all-reduce.

In 'video' / 'text' the fp32 embeddings are what is gathered (not the 16-bit operand) because the exact re-score of the pairs inside
the error band needs both fp32 rows of a pair on the rank that owns the pair; 'video16' moves the pair instead of the row.  choose_sharding() picks the scheme that gathers fewer bytes
(min(Nt, Nv) x K).  S is never gathered.  Uneven shards are padded to the largest shard for the collective and compacted inside
the next captured phase.

`compute` is the per-rank kernel backend (HipBackend below; the gloo/CPU tests inject an oracle-backed stand-in),
so the orchestration is exercised without a GPU.
"""
import torch
import torch.distributed as dist

from . import ops


def shard_bounds(n, world, rank):
    """Contiguous, balanced [lo, hi) -- the first n % world ranks get one extra row."""
    q, r = divmod(n, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


class TorchComm:
    """The collectives of a pass on a torch.distributed group (backend 'nccl' = RCCL; 'gloo' in the CPU tests)."""

    def __init__(self, group=None, force=False):
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.active = self.world > 1 or (force and dist.is_initialized())

    @staticmethod
    def _not_capturing(what, t):
        """The collectives of a pass are EAGER calls between the per-phase HIP graphs (GraphRunner): RCCL under stream capture is not
        proven on this stack, and a collective recorded into a capture by accident would be replayed without its peers.  Fail loudly."""
        if t.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('laff_amd.dist: %s issued while a HIP-graph capture is open on this stream; the collectives of a sharded '
                               'pass run eagerly between the captured phases (GraphRunner.phase)' % what)

    def all_gather(self, out, send, async_op=False):
        self._not_capturing('all_gather', send)
        return dist.all_gather_into_tensor(out, send, group=self.group, async_op=async_op)

    def all_reduce(self, t, op):
        self._not_capturing('all_reduce', t)
        dist.all_reduce(t, op={'max': dist.ReduceOp.MAX, 'sum': dist.ReduceOp.SUM}[op], group=self.group)

    def all_to_all(self, out, send):
        self._not_capturing('all_to_all', send)
        dist.all_to_all_single(out, send, group=self.group)


class EmulatedComm:
    """ONE rank's share of a `world`-rank pass on one device, without a process group (bench.py --emulate-shard): every collective is
    replaced by what it would leave on this rank -- an all-gather copies this rank's block into its slot of the output, whose other
    slots the caller has pre-filled with the peers' rows (the outputs live in the pass's `state` dict under fixed keys); an
    all-reduce combines with `peers[op]`, the peers' combined contribution (a tensor, or absent = nothing to add).  The kernels, their
    shapes and the bytes they move are exactly one rank's; what is missing is the wire time.  Everything here is capturable in a HIP
    graph."""

    def __init__(self, world, rank=0, peers=None):
        self.world, self.rank, self.active, self.group = int(world), int(rank), True, None
        self.peers = peers if peers is not None else {}

    def all_gather(self, out, send, async_op=False):
        n = send.shape[0]
        out[self.rank * n:(self.rank + 1) * n].copy_(send)
        return None

    def all_reduce(self, t, op):
        other = self.peers.get(op)
        if other is not None:
            if op == 'max':
                torch.maximum(t, other, out=t)
            else:
                t.add_(other)

    def all_to_all(self, out, send):
        raise NotImplementedError("EmulatedComm covers the 'video' and 'text' schemes")


def _comm_of(group, comm, force_collectives):
    return comm if comm is not None else TorchComm(group, force_collectives)


class HipBackend:
    """Per-rank compute on liblaff_hip.so."""

    def __init__(self, model, precision='fp16'):
        self.model, self.precision = model, precision
        ops.ctx_prepare_metrics(next(model.parameters()).device)     # scratch allocation outside any graph capture

    def embed_both(self, vis_feats, txt_feats, fused=None):
        """Single-rank shortcut: both towers' FC projections in one grouped launch.  fused (ops.FusedPrepare, from fused_prepare()):
        the two fuse launches also do laff_rank_prepare's work for their rows (videos first: retrieval.embed's order)."""
        from .retrieval import embed
        self._emit_packed(True)
        vl, tl = self.vis_layer(), self.txt_layer()
        if fused is not None:
            vl.rank_side, tl.rank_side = fused.video, fused.text
        try:
            return embed(self.model, vis_feats, txt_feats)
        finally:
            self._emit_packed(False)
            if fused is not None:
                vl.rank_side = tl.rank_side = None

    def embed_video_first(self, vis_feats, txt_feats):
        """embed_both in two steps (retrieval.embed_split): all FC projections + the video fusion now; returns (vis_emb, finish) where
        finish() launches the text fusion and returns txt_emb.  The video tower's operand is not emitted (its rows are gathered in
        fp32 and packed behind the collective); the text tower's is."""
        from .retrieval import embed_split
        self._emit_packed(True)
        try:
            vis_emb, fin_t = embed_split(self.model, vis_feats, txt_feats)
        finally:
            self._emit_packed(False)

        def finish():
            self._emit_packed(True)
            try:
                return fin_t()
            finally:
                self._emit_packed(False)
        return vis_emb, finish

    def fused_prepare(self, Nt, Nv, heads, gt, col0=0):
        """An ops.FusedPrepare when both towers end in a fuse launch that can carry laff_rank_prepare's work (one head of d <= 512,
        fp16 / bf16 operand emitted by the launch), else None (separate rank_prepare launch)."""
        vl, tl = self.vis_layer(), self.txt_layer()
        if not (self._fused_pack(vl) and self._fused_pack(tl)):
            return None
        d = getattr(tl, 'head_dim', None) or getattr(tl, 'embed_dim', None)
        dv = getattr(vl, 'head_dim', None) or getattr(vl, 'embed_dim', None)
        if d is None or d != dv or getattr(tl, 'multi_heads', 1) != heads or getattr(vl, 'multi_heads', 1) != heads:
            return None
        if heads > 1:
            # laff_fuse_packed_rank covers several heads (the heads of a row meet through a scratch + arrival tickets, s_gt64 stays
            # bit-equal), but there it costs what it saves: C1 (8 heads) fuse 1.40 -> 1.75 ms for a 0.33 ms rank_prepare launch, C5
            # 2.03 -> 2.95 for 0.86 -- the separate launch stays
            return None
        if not ops.fused_prepare_eligible(Nt, Nv, heads, int(d), self.precision):
            return None
        return ops.FusedPrepare(Nt, Nv, gt, col0, heads=heads)

    def txt_layer(self):
        return self.model.txt_net.attention_layer

    def vis_layer(self):
        net = self.model.vis_net
        return getattr(net, 'attention_layer', None) or getattr(net, 'vis_attention_layer', None)

    def embed_text(self, txt_feats):
        cap = dict(txt_feats)
        cap.setdefault('caption', None)
        self._emit_packed(True)
        try:
            return self.model.txt_net(cap)
        finally:
            self._emit_packed(False)

    def embed_video(self, vis_feats):
        vis = dict(vis_feats)
        frame_dict = {}
        if 'mask_tensor' in vis:
            frame_dict, vis = vis, {}
        self._emit_packed(True)
        try:
            return self.model.vis_net(vis, vis_frame_feat_dict_input=frame_dict)
        finally:
            self._emit_packed(False)

    def _attention_layers(self):
        return [getattr(net, name) for net in (self.model.vis_net, self.model.txt_net)
                for name in ('attention_layer', 'vis_attention_layer') if hasattr(net, name)]

    def set_unpacked(self, side):
        """side 'txt' | 'vis' | None: that tower's fuse launch does not emit the 16-bit operand (its embeddings are gathered in fp32
        and packed after the collective)."""
        self._unpacked = side

    def _emit_packed(self, on):
        skip = {'txt': [self.txt_layer()], 'vis': [self.vis_layer()]}.get(getattr(self, '_unpacked', None), [])
        for layer in self._attention_layers():
            layer.emit_packed = self.precision if (on and self._fused_pack(layer) and not any(layer is x for x in skip)) else None

    def pack(self, E, layer=None):
        """GEMM operand of an embedding matrix: taken from the fuse launch when it emitted one, else a pack_rows pass."""
        p = getattr(layer, 'last_packed', None) if layer is not None else None
        if p is not None and p.N == E.shape[0]:
            layer.last_packed = None
            return p
        return ops.pack_rows(E, True, 1e-13, self.precision)

    def _fused_pack(self, layer):
        return (self.precision in ('fp16', 'bf16') and layer is not None and hasattr(layer, 'fuse_planes') and
                type(layer).__name__ != 'JustAverage' and getattr(layer, 'fused_pack', True))

    def pack_gathered(self, E, layer=None):
        """GEMM operand of gathered fp32 embedding rows (N, H, d): bit-for-bit what pack() hands over on a single rank -- the fuse
        launch converts its unit-norm rows without re-normalising, pack_rows re-normalises (loss.cosine_sim, loss.py:30-34)."""
        return ops.pack_rows(E, not self._fused_pack(layer), 1e-13, self.precision)

    def sim(self, T, V, heads):
        return ops.sim_gemm(T, V, heads=heads)

    # ---- 'video16' (evaluate_sharded_v16) ----
    def v16_ok(self):
        return self.precision in ('fp16', 'bf16')           # one-plane 16-bit operand

    def v16_rows(self, T):
        """the operand as (N, K * 2) bytes: what is all-gathered"""
        if T.precision not in ('fp16', 'bf16'):
            raise ValueError("'video16' needs a one-plane 16-bit operand, got %r" % T.precision)
        return T.buf[:T.N * T.K * 2].view(T.N, T.K * 2)

    def v16_operand(self, rows2d, N, like):
        return ops.Packed(rows2d.reshape(-1)[:N * like.K * 2], N, like.K, like.precision, like.prescale)

    def v16_band_video(self, Ev, V):
        return ops.rank_band_video(Ev, V)

    def v16_prepare_text(self, Et, T, Ev_all, gt_local):
        return ops.rank_prepare_text(Et, Ev_all, T, gt_local, 0)

    def v16_gemm(self, T_all, V_local, heads, gt, col0, s_gt64, band_t, band_v, want_scores):
        st = ops.banded_state(T_all, V_local, heads, gt, col0, s_gt64, band_t, band_v)
        S = ops.sim_gemm_banded(st, want_scores)
        return S, st

    def v16_export(self, st, S, bounds, col0, cap):
        return ops.rank_export_pairs(st, S, bounds, col0, cap)

    def v16_resolve(self, Et, Ev_all, s_gt64, count, lst):
        return ops.rank_resolve_list(Et, Ev_all, s_gt64, count, lst)

    def prepare(self, Et, Ev, T, V, gt, col0):
        """Exact ground-truth scores of the texts whose video is in [col0, col0 + Nv), error bands, cleared accumulators."""
        return ops.rank_prepare(Et, Ev, T, V, gt, col0)

    def prepare_gathered(self, Et, Ev, T, V, gt, col0, layer):
        """prepare() for a pass in which one side's rows have just been gathered (T or V None): their operand is produced by the
        prepare launch itself instead of a pack_rows pass in front of it -- when the operand is what pack_gathered() would return
        bit for bit (a single-plane 16-bit format made from unit-norm rows without re-normalising); else pack_gathered + prepare."""
        if self.precision in ('fp16', 'bf16') and self._fused_pack(layer):
            return ops.rank_prepare(Et, Ev, T, V, gt, col0, emit_precision=self.precision)
        if T is None:
            T = self.pack_gathered(Et, layer)
        if V is None:
            V = self.pack_gathered(Ev, layer)
        return ops.rank_prepare(Et, Ev, T, V, gt, col0)

    def s_gt_of(self, st):
        return st.s_gt64

    def sim_ranked(self, st, want_scores=True):
        """Score block + exact ground-truth rank counts: banded GEMM epilogue, then the exact re-score of the listed pairs."""
        S = ops.sim_gemm_banded(st, want_scores)
        ops.rank_resolve(st, S)
        return S, st.count

    def sim_ranked_finish(self, st, want_scores=True, out_pinned=None):
        """sim_ranked + finish with the metrics computed by the resolve launch itself (laff_rank_resolve_metrics: nothing -- no
        all-reduce of the counts -- comes between them on a single rank).  Returns (S, count, ranks, metrics or None)."""
        S = ops.sim_gemm_banded(st, want_scores)
        ranks = torch.empty_like(st.count)
        metrics = ops.rank_resolve_metrics(st, S, out_pinned, base=1, ranks_out=ranks)
        return S, st.count, ranks, metrics

    def finish(self, count, out_pinned=None):
        """ranks = count + 1 and the 7 metrics in one launch; returns (ranks, metrics or None when out_pinned is given).
        With out_pinned the caller checks out_pinned[7] (error flag) after its stream sync: check_metrics_flag()."""
        ranks = torch.empty_like(count)
        if out_pinned is not None:
            ops.rank_metrics_async(count, out_pinned, base=1, ranks_out=ranks)
            return ranks, None
        return ranks, ops.rank_metrics(count, base=1, ranks_out=ranks)

    def metrics(self, ranks):
        return ops.rank_metrics(ranks)

    def metrics_async(self, ranks, out_pinned):
        ops.rank_metrics_async(ranks, out_pinned)


class GraphRunner:
    """Runs each LOCAL phase of evaluate_sharded as its own captured HIP graph (first call: capture + replay, later calls:
    replay).  Collectives stay eager between the phases, so nothing RCCL-related is ever captured; what disappears is the
    per-step Python/ctypes issue cost of ~15 kernel launches (0.3-0.4 ms, several times the GPU time of a 1/8 shard)."""

    def __init__(self):
        self.graphs, self.outs = {}, {}

    def __call__(self, name, fn):
        if name not in self.graphs:
            g = torch.cuda.CUDAGraph()
            # thread-local capture mode: the process group's watchdog thread keeps polling its events (hipEventQuery) while this
            # thread captures; under the default global mode that query is an illegal call and aborts the process
            with torch.cuda.graph(g, capture_error_mode='thread_local'):
                out = fn()
            self.graphs[name], self.outs[name] = g, out
        self.graphs[name].replay()
        return self.outs[name]


def _eager(name, fn):
    return fn()


def check_metrics_flag(out_pinned):
    """After the stream sync that makes an async metrics buffer valid: raise if the device flagged the step (a rank < 1, which is
    also how an overflowing pair list of the exact-rank pipeline reports itself)."""
    if float(out_pinned[7]) != 0.0:
        raise RuntimeError('laff_amd: the rank metrics kernel flagged an invalid rank (rank < 1): the pair list of the exact-rank '
                           'pipeline overflowed (degenerate scores: raise pair_cap) or the counts are corrupt')


def gathered_bytes(scheme, Nt, Nv, K, world, pair_bucket_cap=0):
    """Payload bytes that reach ONE rank per pass from the others (all-gathers / all-to-all / all-reduce results), by collective."""
    o = (world - 1) / max(world, 1)
    if scheme == 'video':
        return {'all_gather_text_fp32': int(Nt * K * 4 * o), 'all_reduce_s_gt64': Nt * 8, 'all_reduce_count': Nt * 4}
    if scheme == 'text':
        return {'all_gather_video_fp32': int(Nv * K * 4 * o), 'all_gather_ranks': int(Nt * 4 * o)}
    if scheme == 'video16':
        return {'all_gather_text_16bit': int(Nt * K * 2 * o), 'all_gather_video_fp32': int(Nv * K * 4 * o), 'all_gather_sgt_band': int(Nt * 12 * o),
                'all_to_all_pairs': int(pair_bucket_cap * 8 * (world - 1)), 'all_reduce_count': Nt * 4, 'all_gather_ranks': int(Nt * 4 * o)}
    raise ValueError(scheme)


def choose_sharding(Nt, Nv):
    """The decomposition that gathers fewer embedding rows: 'text' shards (gather the videos) when Nv <= Nt, else 'video'."""
    return 'text' if Nv <= Nt else 'video'


def default_pair_bucket_cap(Nt, world):
    """Slots of one (sender, owner) bucket of 'video16''s pair all-to-all: the even share of 128 pairs per text (the headroom of
    ops.default_pair_cap: C4 lists 2.4 pairs per text, chance-level scores as in C3 ~30), at least 4096, a multiple of 4."""
    return max(4096, (128 * int(Nt) // max(world * world, 1) + 3) & ~3)


def _fused_tail_enabled(Nt):
    """laff_rank_resolve_metrics (ranks + metrics by the resolve launch's last workgroup) instead of laff_rank_resolve +
    laff_rank_metrics_async: one CU reduces all Nt ranks, which beats a second launch up to ~16k queries (C2: 29 vs 31 + a gap us) and
    loses beyond (C4, 40k: 97 vs 82 us).  LAFF_FUSED_TAIL = 0 / 1 forces the choice."""
    import os
    v = os.environ.get('LAFF_FUSED_TAIL')
    if v is not None:
        return v != '0'
    return Nt <= 16384


def _flat_rows(E):
    return E.reshape(E.shape[0], -1)


def _pad_rows(E2, nmax):
    """(n, K) -> contiguous (nmax, K), zero rows appended (equal-sized contributions for all_gather_into_tensor)."""
    if E2.shape[0] == nmax:
        return E2.contiguous()
    pad = torch.zeros((nmax, E2.shape[1]), dtype=E2.dtype, device=E2.device)
    pad[:E2.shape[0]] = E2
    return pad


def _compact(gathered, sizes, nmax, heads):
    """Padded all-gather result (world * nmax, K) -> (N, heads, K / heads): drops the padding rows of uneven shards."""
    K = gathered.shape[1]
    if all(hi - lo == nmax for lo, hi in sizes):
        rows = gathered
    else:
        rows = torch.cat([gathered[r * nmax: r * nmax + (hi - lo)] for r, (lo, hi) in enumerate(sizes)])
    return rows.view(rows.shape[0], heads, K // heads)


def evaluate_sharded(compute, vis_feats_local, txt_feats_local, gt, Nt, Nv, heads, group=None, want_metrics=True,
                     timer=None, want_scores=True, metrics_out=None, runner=None, state=None, force_collectives=False,
                     finish_tag='', comm_impl=None):
    """One pass of the hot path on this rank's shards, videos sharded ('video' scheme of the module docstring).
    gt: (Nt,) int32 GLOBAL video column of every text (replicated).

    runner: None (eager) or a GraphRunner; state: dict that persists across steps (static collective buffers) -- required
    with a GraphRunner.  force_collectives runs the collectives even on a 1-rank group (used to exercise the N > 1 code
    path on a single GPU).  finish_tag names the captured 'finish' phase: callers that alternate between several metrics_out
    buffers (to keep a step in flight while the host reads the previous one) pass a different tag per buffer.
    comm_impl: None (torch.distributed on `group`) or an EmulatedComm (one rank's share of a larger pass on one device).
    Returns dict(S_local (Nt, v1-v0), col0, ranks (Nt,), metrics)."""
    cx = _comm_of(group, comm_impl, force_collectives)
    world, rank, comm = cx.world, cx.rank, cx.active
    v0, v1 = shard_bounds(Nv, world, rank)
    mark = timer.mark if timer is not None else (lambda name: None)
    run = runner if runner is not None else _eager
    state = state if state is not None else {}
    if runner is not None and metrics_out is None and want_metrics:
        raise ValueError('a GraphRunner needs metrics_out (pinned buffer): the synchronising metrics call cannot be captured')
    sizes = [shard_bounds(Nt, world, r) for r in range(world)]
    nmax = max(hi - lo for lo, hi in sizes)
    if hasattr(compute, 'set_unpacked'):
        compute.set_unpacked('txt' if comm else None)
    with torch.no_grad():
        fused_box = [None]
        if not comm and hasattr(compute, 'embed_both'):
            def towers():
                # (single rank: laff_rank_prepare's work rides in the two fuse launches where they can carry it)
                fused = compute.fused_prepare(Nt, Nv, heads, gt, v0) if (hasattr(compute, 'fused_prepare') and runner is None) else None
                if fused is not None:
                    vis_emb, txt_emb = compute.embed_both(vis_feats_local, txt_feats_local, fused)
                    if fused.Et is None or fused.Ev is None:         # (a tower that did not end in the expected fuse launch)
                        fused = None
                else:
                    vis_emb, txt_emb = compute.embed_both(vis_feats_local, txt_feats_local)
                fused_box[0] = fused
                return (txt_emb, compute.pack(txt_emb, compute.txt_layer()), vis_emb, compute.pack(vis_emb, compute.vis_layer()))
            txt_emb, T_all, vis_emb, V_local = run('towers', towers)
            Et_all = txt_emb
            mark('towers')
        else:
            def text_phase():
                txt_emb = compute.embed_text(txt_feats_local)
                return txt_emb, _pad_rows(_flat_rows(txt_emb), nmax)
            txt_emb, send = run('text', text_phase)
            mark('txt_tower')
            work = None
            if comm:
                shape = (world * nmax, send.shape[1])
                if 'gathered' not in state or tuple(state['gathered'].shape) != shape:
                    state['gathered'] = torch.empty(shape, dtype=send.dtype, device=send.device)
                gathered = state['gathered']
                work = cx.all_gather(gathered, send, async_op=True)     # overlaps the video tower

            def video_phase():
                vis_emb = compute.embed_video(vis_feats_local)
                V = compute.pack(vis_emb, compute.vis_layer()) if hasattr(compute, 'vis_layer') else compute.pack(vis_emb)
                return vis_emb, V
            vis_emb, V_local = run('video', video_phase)
            mark('vis_tower')
            if work is not None:
                work.wait()
            mark('all_gather_wait')

        # exact ground-truth score from the shard that owns the column, then one GEMM that writes S and counts ranks
        def prep_phase():
            if comm:
                Et = _compact(gathered, sizes, nmax, heads)
                if hasattr(compute, 'prepare_gathered'):
                    return compute.prepare_gathered(Et, vis_emb, None, V_local, gt, v0, compute.txt_layer())
                T = compute.pack_gathered(Et, compute.txt_layer()) if hasattr(compute, 'txt_layer') else compute.pack_gathered(Et)
            elif hasattr(compute, 'embed_both'):
                if fused_box[0] is not None:
                    return fused_box[0].state()
                Et, T = Et_all, T_all
            else:
                Et = txt_emb
                T = compute.pack(txt_emb, compute.txt_layer()) if hasattr(compute, 'txt_layer') else compute.pack(txt_emb)
            return compute.prepare(Et, vis_emb, T, V_local, gt, v0)
        st = run('prep', prep_phase)
        mark('prep')
        if comm:
            cx.all_reduce(compute.s_gt_of(st), 'max')
            mark('allreduce_s_gt')
        metrics = None
        fused_tail = (not comm and hasattr(compute, 'sim_ranked_finish') and (metrics_out is not None or want_metrics) and
                      _fused_tail_enabled(Nt))
        if fused_tail:
            # one rank: GEMM, then ONE launch that re-scores the listed pairs and ends with the ranks + metrics
            S_local, count, ranks, metrics = run('sim_finish' + finish_tag, lambda: compute.sim_ranked_finish(st, want_scores, metrics_out))
            mark('sim_gemm')
            mark('rank')
            mark('metrics')
            return {'S_local': S_local, 'col0': v0, 'ranks': ranks, 'metrics': metrics, 'vis_emb': vis_emb, 'txt_emb': txt_emb,
                    'rank_state': st}
        S_local, count = run('sim', lambda: compute.sim_ranked(st, want_scores))
        mark('sim_gemm')
        if comm:
            # an overflowing pair list poisons count[0] with -(2^26) on every rank it happens on (rank.hip: rank_resolve_kernel); the
            # SUM of up to 16 such poisons stays negative, so the rank < 1 flag of the metrics kernel still trips after the reduction
            cx.all_reduce(count, 'sum')
            mark('allreduce_count')

        if hasattr(compute, 'finish') and (metrics_out is not None or want_metrics):
            # one launch: ranks = count + 1 and the metrics (no host sync when metrics_out is given)
            if metrics_out is not None:
                ranks = run('finish' + finish_tag, lambda: compute.finish(count, metrics_out)[0])
            else:
                ranks, metrics = compute.finish(count)
            mark('rank')
        else:
            def finish():
                ranks = count + 1
                if metrics_out is not None:
                    compute.metrics_async(ranks, metrics_out)     # no host sync: the caller reads metrics_out after one
                return ranks
            ranks = run('finish' + finish_tag, finish)
            mark('rank')
            if metrics_out is None and want_metrics:
                metrics = compute.metrics(ranks)
        mark('metrics')
    return {'S_local': S_local, 'col0': v0, 'ranks': ranks, 'metrics': metrics, 'vis_emb': vis_emb, 'txt_emb': txt_emb,
            'rank_state': st}


def evaluate_sharded_by_text(compute, vis_feats_local, txt_feats_local, gt, Nt, Nv, heads, group=None, want_metrics=True,
                             want_scores=True, metrics_out=None, runner=None, state=None, force_collectives=False,
                             finish_tag='', timer=None, comm_impl=None):
    """The 'text' scheme of the module docstring: rank g owns texts [t0, t1) end to end and the ROW block S[t0:t1, :]; videos are
    split for the embedding stage only and ONE all-gather of the fp32 VIDEO embeddings (Nv x K: a quarter of the text side at C4)
    gives every rank all videos.  Every text then meets its ground-truth video locally, so neither the MAX all-reduce of s_gt
    nor the SUM all-reduce of the counts is needed; the ranks (Nt int32) are all-gathered for the replicated metrics.
    Returns dict(S_local (t1-t0, Nv), row0, ranks (Nt,), metrics)."""
    cx = _comm_of(group, comm_impl, force_collectives)
    world, rank, comm = cx.world, cx.rank, cx.active
    t0, t1 = shard_bounds(Nt, world, rank)
    mark = timer.mark if timer is not None else (lambda name: None)
    run = runner if runner is not None else _eager
    state = state if state is not None else {}
    if runner is not None and metrics_out is None and want_metrics:
        raise ValueError('a GraphRunner needs metrics_out (pinned buffer): the synchronising metrics call cannot be captured')
    vsizes = [shard_bounds(Nv, world, r) for r in range(world)]
    tsizes = [shard_bounds(Nt, world, r) for r in range(world)]
    vmax = max(hi - lo for lo, hi in vsizes)
    tmax = max(hi - lo for lo, hi in tsizes)
    if hasattr(compute, 'set_unpacked'):
        compute.set_unpacked('vis' if comm else None)
    with torch.no_grad():
        if comm and hasattr(compute, 'embed_video_first'):
            # Every FC projection of both towers in one launch, the video fusion, then the video rows leave for the other ranks
            # (asynchronously) while the text side is fused: the gather's first ~20-50 us (the text fusion of a 1/8 .. 1/2 shard) are off
            # the critical path at no extra launch.
            fin_box = [None]

            def towers_a():
                vis_emb, fin_box[0] = compute.embed_video_first(vis_feats_local, txt_feats_local)
                return vis_emb, _pad_rows(_flat_rows(vis_emb), vmax)
            vis_emb, send = run('towers_ta', towers_a)
            mark('vis_tower')
            shape = (world * vmax, send.shape[1])
            if 'gathered_v' not in state or tuple(state['gathered_v'].shape) != shape:
                state['gathered_v'] = torch.empty(shape, dtype=send.dtype, device=send.device)
            gathered = state['gathered_v']
            work = cx.all_gather(gathered, send, async_op=True)

            def towers_b():
                txt_emb = fin_box[0]()
                return txt_emb, (compute.pack(txt_emb, compute.txt_layer()) if hasattr(compute, 'txt_layer') else compute.pack(txt_emb))
            txt_emb, T_local = run('towers_tb', towers_b)
            V_local = None
            mark('towers')
            if work is not None:
                work.wait()
            mark('all_gather_wait')
        else:
            def towers():
                if hasattr(compute, 'embed_both'):
                    vis_emb, txt_emb = compute.embed_both(vis_feats_local, txt_feats_local)
                else:
                    txt_emb, vis_emb = compute.embed_text(txt_feats_local), compute.embed_video(vis_feats_local)
                T_local = compute.pack(txt_emb, compute.txt_layer()) if hasattr(compute, 'txt_layer') else compute.pack(txt_emb)
                if comm:
                    return txt_emb, vis_emb, T_local, None, _pad_rows(_flat_rows(vis_emb), vmax)
                V_local = compute.pack(vis_emb, compute.vis_layer()) if hasattr(compute, 'vis_layer') else compute.pack(vis_emb)
                return txt_emb, vis_emb, T_local, V_local, None
            txt_emb, vis_emb, T_local, V_local, send = run('towers_t', towers)
            mark('towers')
            if comm:
                shape = (world * vmax, send.shape[1])
                if 'gathered_v' not in state or tuple(state['gathered_v'].shape) != shape:
                    state['gathered_v'] = torch.empty(shape, dtype=send.dtype, device=send.device)
                gathered = state['gathered_v']
                cx.all_gather(gathered, send)
            mark('all_gather_wait')
        # this rank's slice of the ground-truth columns lives in `state`: a captured phase reads it at a fixed address on every
        # replay, and it is refreshed from `gt` on every step (outside the captured phase) like the 'video' scheme reads gt live
        if 'gt_local' not in state or state['gt_local'].numel() != t1 - t0 or state['gt_local'].device != gt.device:
            state['gt_local'] = torch.empty(t1 - t0, dtype=gt.dtype, device=gt.device)
        gt_local = state['gt_local']
        gt_local.copy_(gt[t0:t1])

        def rank_phase():
            if comm:
                Ev = _compact(gathered, vsizes, vmax, heads)
                V = None if hasattr(compute, 'prepare_gathered') else (
                    compute.pack_gathered(Ev, compute.vis_layer()) if hasattr(compute, 'vis_layer') else compute.pack_gathered(Ev))
            else:
                Ev, V = vis_emb, V_local
            if V is None:
                st = compute.prepare_gathered(txt_emb, Ev, T_local, None, gt_local, 0, compute.vis_layer())
            else:
                st = compute.prepare(txt_emb, Ev, T_local, V, gt_local, 0)
            S_local, count = compute.sim_ranked(st, want_scores)
            mine = (count + 1).to(torch.int32)
            if comm and mine.numel() != tmax:
                pad = torch.ones(tmax, dtype=torch.int32, device=mine.device)
                pad[:mine.numel()] = mine
                mine = pad
            return S_local, mine.contiguous(), st
        S_local, mine, st = run('rank_t', rank_phase)
        mark('sim_gemm')
        if comm:
            if 'gathered_r' not in state or state['gathered_r'].numel() != world * tmax:
                state['gathered_r'] = torch.empty(world * tmax, dtype=torch.int32, device=mine.device)
            all_ranks = state['gathered_r']
            cx.all_gather(all_ranks, mine)
            mark('allgather_ranks')
        else:
            all_ranks = mine

        def finish():
            if comm and not all(hi - lo == tmax for lo, hi in tsizes):
                ranks = torch.cat([all_ranks[r * tmax: r * tmax + (hi - lo)] for r, (lo, hi) in enumerate(tsizes)])
            else:
                ranks = all_ranks[:Nt]
            if metrics_out is not None:
                compute.metrics_async(ranks, metrics_out)
            return ranks
        ranks = run('finish_t' + finish_tag, finish)
        mark('rank')
        metrics = None
        if metrics_out is None and want_metrics:
            metrics = compute.metrics(ranks)
        mark('metrics')
    return {'S_local': S_local, 'row0': t0, 'ranks': ranks, 'metrics': metrics, 'vis_emb': vis_emb, 'txt_emb': txt_emb,
            'rank_state': st}


def _all_gather_rows(x2d, nmax, world, comm, cx, state, key, async_op=False):
    """all-gather of equally padded row blocks; returns (gathered (world * nmax, cols) or x2d itself, work or None)"""
    if not comm:
        return x2d, None
    send = _pad_rows(x2d, nmax)
    shape = (world * nmax, send.shape[1])
    if key not in state or tuple(state[key].shape) != shape or state[key].dtype != send.dtype:
        state[key] = torch.empty(shape, dtype=send.dtype, device=send.device)
    work = cx.all_gather(state[key], send, async_op=async_op)
    return state[key], (work if async_op else None)


def _compact2d(gathered, sizes, nmax):
    if all(hi - lo == nmax for lo, hi in sizes):
        return gathered
    return torch.cat([gathered[r * nmax: r * nmax + (hi - lo)] for r, (lo, hi) in enumerate(sizes)])


def evaluate_sharded_v16(compute, vis_feats_local, txt_feats_local, gt, Nt, Nv, heads, group=None, want_metrics=True, timer=None,
                         want_scores=True, metrics_out=None, runner=None, state=None, force_collectives=False, finish_tag='',
                         pair_bucket_cap=None, comm_impl=None):
    """The 'video16' scheme of the module docstring: rank g owns videos [v0, v1) and the column block S[:, v0:v1] as in
    evaluate_sharded, but the text side crosses the links as the 16-bit operand; exact re-scores happen at the text owners.
    pair_bucket_cap: slots of one (sender, owner) bucket of the pair all-to-all (default_pair_bucket_cap: the even share of 128 pairs
    per text, at least 4096).  A bucket that fills up poisons count[0]: the pass ends in check_metrics_flag's RuntimeError (or, with
    want_metrics=False, in a rank < 1) -- call again with a larger pair_bucket_cap; `pair_fill` in the result tells how full they were.
    Needs a one-plane 16-bit operand (fp16 / bf16): ValueError otherwise.
    S_local: the in-band pairs are re-scored at the owner of their TEXT row, which holds no part of S, so S_local keeps the 16-bit
    GEMM's value for them (inside the band of the exact score) -- only the ground-truth entries carry the exact score.  Ranks
    recounted from S_local can therefore differ from the exact `ranks` returned here by the pairs inside the band; the 'video' and
    'text' schemes patch S and do agree.
    Returns dict(S_local (Nt, v1 - v0), col0, ranks (Nt,), metrics, gathered_bytes)."""
    if hasattr(compute, 'v16_ok') and not compute.v16_ok():
        raise ValueError("evaluate_sharded_v16 gathers a one-plane 16-bit operand: precision must be 'fp16' or 'bf16', not %r"
                         % getattr(compute, 'precision', None))
    cx = _comm_of(group, comm_impl, force_collectives)
    world, rank, comm = cx.world, cx.rank, cx.active
    mark = timer.mark if timer is not None else (lambda name: None)
    run = runner if runner is not None else _eager
    state = state if state is not None else {}
    if runner is not None and metrics_out is None and want_metrics:
        raise ValueError('a GraphRunner needs metrics_out (pinned buffer): the synchronising metrics call cannot be captured')
    v0, v1 = shard_bounds(Nv, world, rank)
    t0, t1 = shard_bounds(Nt, world, rank)
    tsizes = [shard_bounds(Nt, world, r) for r in range(world)]
    vsizes = [shard_bounds(Nv, world, r) for r in range(world)]
    tmax = max(hi - lo for lo, hi in tsizes)
    vmax = max(hi - lo for lo, hi in vsizes)
    if pair_bucket_cap is None:
        pair_bucket_cap = default_pair_bucket_cap(Nt, world)
    cap = (int(pair_bucket_cap) + 3) & ~3
    if hasattr(compute, 'set_unpacked'):
        compute.set_unpacked(None)
    with torch.no_grad():
        dev = gt.device
        if 'bounds' not in state or state['bounds'].numel() != world + 1 or state['bounds'].device != dev:
            state['bounds'] = torch.tensor([lo for lo, _ in tsizes] + [Nt], dtype=torch.int32, device=dev)
        if 'gt_local' not in state or state['gt_local'].numel() != t1 - t0 or state['gt_local'].device != dev:
            state['gt_local'] = torch.empty(t1 - t0, dtype=gt.dtype, device=dev)
        state['gt_local'].copy_(gt[t0:t1])
        gt_local = state['gt_local']

        # ---- towers; the text operand and the video rows start travelling while the other tower runs ----
        def text_phase():
            txt_emb = compute.embed_text(txt_feats_local)
            T = compute.pack(txt_emb, compute.txt_layer()) if hasattr(compute, 'txt_layer') else compute.pack(txt_emb)
            return txt_emb, T, compute.v16_rows(T)
        txt_emb, T_local, t_rows = run('text16', text_phase)
        mark('txt_tower')
        t_all, w1 = _all_gather_rows(t_rows, tmax, world, comm, cx, state, 'g_t16', async_op=True)

        def video_phase():
            vis_emb = compute.embed_video(vis_feats_local)
            V = compute.pack(vis_emb, compute.vis_layer()) if hasattr(compute, 'vis_layer') else compute.pack(vis_emb)
            return vis_emb, V, compute.v16_band_video(vis_emb, V), _flat_rows(vis_emb)
        vis_emb, V_local, band_v, v_rows = run('video16', video_phase)
        mark('vis_tower')
        v_all, w2 = _all_gather_rows(v_rows, vmax, world, comm, cx, state, 'g_v32', async_op=True)
        for w in (w1, w2):
            if w is not None:
                w.wait()
        mark('all_gather_wait')

        # ---- the text owner: exact ground-truth scores + bands of its rows -> everybody ----
        def owner_phase():
            Ev_all = _compact(v_all, vsizes, vmax, heads) if comm else vis_emb
            s_gt64, band_t = compute.v16_prepare_text(txt_emb, T_local, Ev_all, gt_local)
            pay = torch.empty((t1 - t0, 3), dtype=torch.float32, device=s_gt64.device)
            pay[:, :2] = s_gt64.view(torch.float32).view(-1, 2)
            pay[:, 2] = band_t[:t1 - t0]
            return Ev_all, s_gt64, band_t, pay
        Ev_all, s_gt64_l, band_t_l, pay = run('owner16', owner_phase)
        mark('prep')
        pay_all, _ = _all_gather_rows(pay, tmax, world, comm, cx, state, 'g_pay')
        mark('allgather_sgt_band')

        # ---- the video owner: banded GEMM of ALL texts x its videos; pairs inside the band -> buckets per text owner ----
        def gemm_phase():
            if comm:
                rows = _compact2d(t_all, tsizes, tmax)
                T_all = compute.v16_operand(rows, Nt, T_local)
                p = _compact2d(pay_all, tsizes, tmax)
                s_all = p[:, :2].contiguous().view(torch.float64).view(-1)
                b_all = torch.zeros(Nt + 4, dtype=torch.float32, device=p.device)
                b_all[:Nt] = p[:, 2]
            else:
                T_all, s_all, b_all = T_local, s_gt64_l, band_t_l
            return compute.v16_gemm(T_all, V_local, heads, gt, v0, s_all, b_all, band_v, want_scores)
        S_local, st = run('gemm16', gemm_phase)
        mark('sim_gemm')
        send, fill = run('export16', lambda: compute.v16_export(st, S_local, state['bounds'], v0, cap))
        mark('export_pairs')
        count = st.count
        if comm:
            if 'recv' not in state or state['recv'].numel() != 4 + 2 * world * cap:
                state['recv'] = torch.empty(4 + 2 * world * cap, dtype=torch.int32, device=send.device)
                state['recv'][:4] = torch.tensor([0, 0, world * cap, 4], dtype=torch.int32, device=send.device)
            lst = state['recv']
            cx.all_to_all(lst[4:].view(world, cap, 2), send)
            cx.all_reduce(count, 'sum')          # (a full bucket poisons count[0]: stays negative)
            mark('alltoall_pairs')
        else:
            # one rank, no collectives: the list lives in `state` (a captured resolve phase reads it at a fixed address on every replay)
            # and is refilled from this step's buckets INSIDE that phase
            if 'lst_local' not in state or state['lst_local'].numel() != 4 + 2 * world * cap or state['lst_local'].device != send.device:
                state['lst_local'] = torch.empty(4 + 2 * world * cap, dtype=torch.int32, device=send.device)
                state['lst_local'][:4] = torch.tensor([0, 0, world * cap, 4], dtype=torch.int32, device=send.device)
            lst = state['lst_local']

        # ---- the text owner: exact re-score of the pairs of its rows; ranks -> everybody ----
        def resolve_phase():
            if not comm:
                lst[4:].copy_(send.reshape(-1))
            mine = count[t0:t1].clone()
            compute.v16_resolve(txt_emb, Ev_all, s_gt64_l, mine, lst)
            r = (mine + 1).to(torch.int32)
            if comm and r.numel() != tmax:
                pad = torch.ones(tmax, dtype=torch.int32, device=r.device)
                pad[:r.numel()] = r
                r = pad
            return r.contiguous()
        mine = run('resolve16', resolve_phase)
        if comm:
            if 'g_ranks' not in state or state['g_ranks'].numel() != world * tmax:
                state['g_ranks'] = torch.empty(world * tmax, dtype=torch.int32, device=mine.device)
            all_ranks = state['g_ranks']
            cx.all_gather(all_ranks, mine)
            mark('allgather_ranks')
        else:
            all_ranks = mine

        def finish():
            if comm and not all(hi - lo == tmax for lo, hi in tsizes):
                ranks = torch.cat([all_ranks[r * tmax: r * tmax + (hi - lo)] for r, (lo, hi) in enumerate(tsizes)])
            else:
                ranks = all_ranks[:Nt]
            if metrics_out is not None:
                compute.metrics_async(ranks, metrics_out)
            return ranks
        ranks = run('finish16' + finish_tag, finish)
        mark('rank')
        metrics = None
        if metrics_out is None and want_metrics:
            metrics = compute.metrics(ranks)
        mark('metrics')
    K = txt_emb.reshape(txt_emb.shape[0], -1).shape[1]
    return {'S_local': S_local, 'col0': v0, 'ranks': ranks, 'metrics': metrics, 'vis_emb': vis_emb, 'txt_emb': txt_emb, 'rank_state': st,
            'pair_fill': fill, 'gathered_bytes': gathered_bytes('video16', Nt, Nv, K, world, cap)}
