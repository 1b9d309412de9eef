"""Training-step driver for the HIP SeqPAN path: static device buffers, the whole step
(forward + backward + clip + AdamWD) enqueued through the C ABI and - single GPU - replayed as ONE hipGraph.

Equivalent of the loop body of /root/reference/utils/runner_utils.py:144-147 (feed_dict upload + sess.run).
"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

from . import dist as hdist
from . import lib


class _Step:
    """One launchable step: the ABI structs over one set of feed and fetch buffers, the job table of its weight-gradient launch and -
    once captured - its launcher.  The static mode (set_batch) owns one, the device-fed mode (set_batch_device) a cache of them."""
    __slots__ = ('bt', 'lab', 'out', 'table', 'tables_ready', 'seen', 'nograph', 'graph', 'drop')

    def __init__(self, bt, lab, out, table):
        self.bt, self.lab, self.out = bt, lab, out
        # the step's OWN job table (hual_run_opts.dw_table), never in the workspace: that is shared with every other user of the
        # model (model.forward at another shape, a second Trainer, the other padded shapes of a loop) and static_tables must not
        # depend on what they leave there.  tables_ready: a backward on these buffers HAS written it - from then on nothing rewrites
        # it (five launches fewer per step, eager or replayed)
        self.table, self.tables_ready = table, False
        self.seen = 0             # eager launches of this step so far
        self.nograph = False      # a capture of it was refused: eager launches for good
        self.graph = None         # the captured launcher: one CUDAGraph, or the three segment graphs of a data-parallel step ...
        self.drop = None          # ... and the drop rate recorded in it


# Trainer.dp_launch of a replayed data-parallel step, by "its launcher is a list of segment graphs"
_DP_LAUNCH = {True: 'three hipGraphs of the launches, the two collectives eager between them',
              False: 'hipGraph with the collectives captured'}


class Trainer:
    def __init__(self, model, world=1, use_graph=True, force_dp=False):
        self.m = model
        self.world = world
        self.dp = world > 1 or force_dp          # force_dp: run the data-parallel code path on one rank (tests)
        self.use_graph = use_graph and not self.dp
        self.dp_graph = use_graph and self.dp     # data-parallel step as graph(s): _dp_mode
        self.dp_launch = 'eager'                  # how the last data-parallel step was launched: eager / segment graphs / one graph
        self._prezero_token = ctypes.c_uint64(0)
        self.shape = None
        self._lib = lib.load()
        self._cur = None             # the _Step that _opts / _forward / _backward / step work on
        # device-fed mode (set_batch_device): per-shape cache of steps, outputs at the largest shape seen
        self.dynamic = False
        # per-shape cache of the device-fed mode.  The reference's own annotations give ~340 distinct (L, C) padded shapes per
        # ActivityNet epoch at batch 16 and more with varying T (tests/golden/lengths_anet.npz): the bound is far above that (an entry
        # is a few ctypes structs, a 60 KB job table and - once captured - a hipGraphExec of ~55 kernel nodes), evictions are counted
        self.cache_limit = 8192
        self.capture_after = 1       # sightings of a shape that are launched eagerly before its step graph is captured
        self._cache = {}
        self._out_cap = None
        self._dp_bufs = {}
        self._cap_stream = None
        self._host_denom = None      # data-parallel epoch loop: the matching-loss denominator computed on the host (shard_plan)
        self._loop = None            # run_epoch: ids / cursor / span bank of the device-side epoch position, the dataset, the current views
        self._loop_state = None
        self._feeds = self._feed_owner = None      # run_epoch: the max-shape feed buffers and the dataset they were made for
        self._table_bytes = int(self._lib.hual_seqpan_dw_table_bytes())
        if self.dp and world > 1:
            hdist.enable_custom_allreduce(model.grads)      # collective; a no-op unless HUAL_ALLREDUCE=custom (default: RCCL)
        self.stats = dict(eager=0, captured=0, replayed=0, evicted=0, capture_failed=0)

    # the current step's ABI structs and launcher, for readers outside (graph: None until that step has been captured)
    bt = property(lambda self: self._cur.bt)
    lab = property(lambda self: self._cur.lab)
    out = property(lambda self: self._cur.out)
    graph = property(lambda self: None if self._cur is None else self._cur.graph)

    def _new_step(self):
        """a _Step over the feed and fetch tensors the trainer points at now"""
        return _Step(lib.batch_struct(self.video, self.lens, self.word_ids, self.char_ids),
                     lib.labels_struct(self.y1, self.y2, self.match, self.inner),
                     lib.outputs_struct(self.start_logits, self.end_logits, self.match_scores, self.start_index, self.end_index,
                                        self.loss_terms),
                     torch.empty(self._table_bytes, dtype=torch.uint8, device=self.m.device))

    # ------------------------------------------------------------------ static batch buffers
    def set_batch(self, video, lens, word_ids, char_ids, y1, y2, match_labels, inner_labels, video_dtype=torch.float32):
        """video_dtype=torch.bfloat16 keeps the clip features in HBM as bfloat16 (hual_batch.video_dtype; the float32 input is
        rounded once here)"""
        m, dev = self.m, self.m.device
        B, T, V = np.shape(video)
        L, C = np.shape(word_ids)[1], np.shape(char_ids)[2]
        # model.py:31 pads to the longest clip of the batch.  A data-parallel shard must be padded to the longest clip of the
        # GLOBAL batch to reproduce the single-process numbers (the reference's conv_block does not mask: rows behind a clip's
        # end feed its last valid rows, so the results depend on the padded length) - hence T >= max(lens) there.
        if int(np.max(lens)) != T and not (self.dp and int(np.max(lens)) < T):
            raise ValueError('video T must equal max(video_seq_len) - model.py:31')
        if self.dp and os.environ.get('HUAL_DP_SKIP_T_CHECK') != '1':
            hdist.check_padded_length(int(np.max(lens)), T)      # raises on EVERY rank together
        shape = (B, T, L, C, video_dtype)
        if shape != self.shape or self.dynamic:
            self.dynamic = False
            self.shape = shape
            f32, i32 = torch.float32, torch.int32
            self.video = torch.empty(B, T, V, device=dev, dtype=video_dtype)
            self.lens = torch.empty(B, device=dev, dtype=i32)
            self.word_ids = torch.empty(B, L, device=dev, dtype=i32)
            self.char_ids = torch.empty(B, L, C, device=dev, dtype=i32)
            self.y1 = torch.empty(B, T, device=dev, dtype=f32)
            self.y2 = torch.empty(B, T, device=dev, dtype=f32)
            self.match = torch.empty(B, T, device=dev, dtype=i32)
            self.inner = torch.empty(B, T, device=dev, dtype=f32)
            self.start_logits = torch.empty(B, T, device=dev)
            self.end_logits = torch.empty(B, T, device=dev)
            self.match_scores = torch.empty(B, T, 4, device=dev)
            self.start_index = torch.empty(B, device=dev, dtype=torch.int64)
            self.end_index = torch.empty(B, device=dev, dtype=torch.int64)
            self.loss_terms = torch.zeros(4, device=dev)
            self.ws = m._workspace(B, T, L, C)
            self._cache.clear()       # (entries of an earlier device-fed phase hold the addresses of the old fetch tensors)
            self._out_cap = None
            self._cur = self._new_step()
            if self.dp:
                self._alloc_dp(B)

        def put(dst, src, dt):
            dst.copy_(torch.as_tensor(np.ascontiguousarray(src), dtype=dt), non_blocking=False)
        put(self.video, video, torch.float32)        # copy_ converts to the buffer's dtype
        put(self.lens, lens, torch.int32)
        put(self.word_ids, word_ids, torch.int32)
        put(self.char_ids, char_ids, torch.int32)
        put(self.y1, y1, torch.float32)
        put(self.y2, y2, torch.float32)
        put(self.match, match_labels, torch.int32)
        put(self.inner, inner_labels, torch.float32)
        self._update_match_denominator()

    def _alloc_dp(self, B):
        """static buffers of the data-parallel exchange: [that | vhat] of the local / all samples, the [Bg,Bg] scratch of the
        alignment loss, its value, and the device scalar holding the matching-loss denominator.  One set per local batch size, kept for
        the trainer's lifetime: the segment graphs of a padded shape hold their addresses (an epoch's ragged last batch comes back
        every epoch)."""
        if B not in self._dp_bufs:
            dev, Bg = self.m.device, B * self.world
            self._dp_bufs[B] = (torch.empty(2 * Bg * Bg + Bg, device=dev), torch.empty(Bg, 256, device=dev), torch.zeros(1, device=dev),
                                torch.zeros(1, device=dev))
        self.align_scratch, self.feat_all, self.align_loss, self.denom_dev = self._dp_bufs[B]

    def _update_match_denominator(self):
        """exact data parallel: the masked matching loss divides by the GLOBAL valid-frame count; every rank
        uses n_global / world (+1e-12 of layers.py:173 on the global count) so that the rank average is the global masked
        mean.  Device side: sum of the lengths -> all-reduce -> scalar the kernels read (hual_run_opts.match_denom_dev);
        no host round trip, so it can sit in front of every batch of a device-fed loop."""
        self.match_denom = 0.0
        if not self.dp:
            return
        if self._host_denom is not None:
            # the epoch loop knows the global batch's lengths on the host: no collective - but the value still travels through the DEVICE
            # scalar (one fill launch): a step's options must not change from batch to batch of a padded shape, they are baked into
            # that shape's segment graphs (by value the first batch's denominator would be replayed for every later one)
            self.denom_dev.fill_(float(self._host_denom))
            return
        torch.sum(self.lens.to(torch.float32), dim=0, keepdim=True, out=self.denom_dev)
        hdist.allreduce_sum_(self.denom_dev)
        self.denom_dev.add_(1e-12).div_(float(self.world))

    def set_batch_device(self, feeds):
        """Point the step at feeds that already live on the device (DeviceDataset.assemble): no host copy, no upload.
        The padded shape changes from batch to batch (runner_utils.py:139-159: T / L / C are maxima over the batch), so this
        mode keeps a small cache keyed by (shape, feed addresses): the structs of the C ABI, and - single GPU, use_graph - a
        hipGraph of the whole step per shape.  A shape is launched eagerly the first time it is seen (first-use attribute calls
        happen outside any capture) and captured the second time; with static feed buffers (DeviceDataset.feed_buffers) and
        the one workspace of SeqPAN.reserve() every later batch of that shape is ONE graph launch.  Nothing is allocated,
        filled or synchronised when the shape changes."""
        m = self.m
        B, T, V = feeds['video'].shape
        L, C = feeds['word_ids'].shape[1], feeds['char_ids'].shape[2]
        self.dynamic = True
        self.video, self.lens, self.word_ids, self.char_ids = (feeds[k] for k in ('video', 'video_seq_len', 'word_ids', 'char_ids'))
        self.y1, self.y2, self.match, self.inner = (feeds[k] for k in ('y1', 'y2', 'match_labels', 'inner_labels'))
        vdt = self.video.dtype
        self.shape = (B, T, L, C, vdt)
        self._ensure_outputs(B, T)
        self.ws = m._workspace(B, T, L, C)
        self.start_logits = self._out_flat[:B * T].view(B, T)
        self.end_logits = self._out_flat[self._out_cap[0] * self._out_cap[1]:][:B * T].view(B, T)
        self.match_scores = self._out_flat[2 * self._out_cap[0] * self._out_cap[1]:][:B * T * 4].view(B, T, 4)
        self.start_index, self.end_index = self.spans[0, :B], self.spans[1, :B]
        lp = self._loop
        key = (B, T, L, C, vdt, self.ws.data_ptr(), self._out_flat.data_ptr(), self.loss_terms.data_ptr(), self.spans.data_ptr(),
               0 if lp is None else (lp['ids'].data_ptr(), lp['cursor'].data_ptr(), lp['bank'].data_ptr(), lp['ds'].soft_address())) + tuple(
            t.data_ptr() for t in (self.video, self.lens, self.word_ids, self.char_ids, self.y1, self.y2, self.match, self.inner))
        s = self._cache.pop(key, None)                           # (re-)inserted below: most recently used last
        if s is None:
            if len(self._cache) >= self.cache_limit:            # bounded: drop the least recently used shape
                self._cache.pop(next(iter(self._cache)))
                self.stats['evicted'] += 1
            s = self._new_step()
        self._cache[key] = s
        self._cur = s
        if self.dp:
            self._alloc_dp(B)
        self._update_match_denominator()

    def _ensure_outputs(self, B, T):
        """fetch tensors of the device-fed mode: one allocation for the largest (B, T) seen (growing it drops the cached graphs -
        they hold the old addresses; run_epoch reserves the set's maximum up front, so a loop never grows it); spans as ONE [2, B]
        tensor so a loop can bank both with one copy"""
        cap = self._out_cap
        if cap is not None and B <= cap[0] and T <= cap[1]:
            return
        Bc, Tc = max(B, cap[0] if cap else 0), max(T, cap[1] if cap else 0)
        dev = self.m.device
        self._out_cap = (Bc, Tc)
        self._out_flat = torch.empty(6 * Bc * Tc, device=dev)
        self.spans = torch.zeros(2, Bc, device=dev, dtype=torch.int64)
        self.loss_terms = torch.zeros(4, device=dev)
        self._cache.clear()

    def reserve(self, B, T, L, C):
        """size workspace and fetch tensors for the largest batch of a loop up front (no growth inside it)"""
        self.m.reserve(B, T, L, C)
        self._ensure_outputs(B, T)

    # ------------------------------------------------------------------ one step
    def _opts(self, drop_rate, align_external, defer_loss=True):
        """defer_loss: the forward leaves the closing of the loss to the backward's matching-head launch (one launch fewer per step,
        hual_run_opts.deferred_loss_terms) - for a forward that IS followed by its backward; False for a forward on its own"""
        # static_tables: all buffers of a step are static, so after one backward on them its job table stays valid
        # (hual_run_opts.static_tables)
        s = self._cur
        return lib.hual_run_opts(float(drop_rate), lib.ptr(self.m.rng_state).value, float(self.match_denom),
                                 int(align_external),
                                 1 if (s.tables_ready and not os.environ.get('HUAL_NO_STATIC_TABLES')) else 0,
                                 lib.ptr(self.denom_dev).value if self.dp else None, 0,
                                 # the forward's first launch zeroes the gradient bucket (one launch fewer in backward); the
                                 # host word is the receipt the backward call checks and clears (hual_run_opts.prezero_token)
                                 lib.ptr(self.m.grads).value, ctypes.addressof(self._prezero_token),
                                 lib.ptr(self.loss_terms).value if defer_loss else None,
                                 lib.ptr(s.table).value, self._table_bytes)

    def _forward(self, opts):
        m, s = self.m, self._cur
        lib.check(self._lib.hual_seqpan_forward(
            ctypes.byref(m.cfg), lib.ptr(m.params), lib.ptr(m.word_table), ctypes.byref(s.bt), ctypes.byref(s.lab),
            ctypes.byref(s.out), ctypes.byref(opts), lib.ptr(self.ws), self.ws.numel(), lib.stream_ptr()))

    def _backward(self, opts):
        m, s = self.m, self._cur
        lib.check(self._lib.hual_seqpan_backward(
            ctypes.byref(m.cfg), lib.ptr(m.params), lib.ptr(m.word_table), ctypes.byref(s.bt), ctypes.byref(s.lab),
            ctypes.byref(opts), lib.ptr(m.grads), lib.ptr(self.ws), self.ws.numel(), lib.stream_ptr()))
        # the launches that write the job table are enqueued - unless this call only recorded them: then the graph's first replay
        # runs them (_replay)
        if not s.tables_ready and not torch.cuda.is_current_stream_capturing():
            s.tables_ready = True

    def _adam(self, prescale):
        # the Philox offset of the dropout stream advances in the same launch (rng_state[2] += 1) ...
        lp = self._loop
        loop = None
        if lp is not None:
            # ... and so does the epoch loop's device-side position: the step's spans go to their place in the bank, the cursor moves on
            nsp = self.spans.numel()
            loop = (lp['cursor'], self.spans, lp['bank'], nsp, int(self.shape[0]), nsp)
        # ... and so do the averaged weights of a model that keeps them (train.ema_decay): SeqPAN.optimizer_launch picks the entry point
        self.m.optimizer_launch(prescale, rng=True, loop=loop)

    def _enqueue_assembly(self):
        """epoch loop: the batch-assembly launch is the first launch of the step (and of the step's graph)"""
        lp = self._loop
        if lp is not None:
            lp['ds'].enqueue_assemble_cursor(lp['views'], lp['ids'], lp['cursor'])

    def _enqueue_single(self, drop_rate):
        self._enqueue_assembly()
        opts = self._opts(drop_rate, 0)
        self._forward(opts)
        self._backward(opts)
        self._adam(1.0)

    # one data-parallel step = three runs of our own launches with a collective between them
    def _dp_part_a(self, opts):
        self._enqueue_assembly()
        self._forward(opts)

    def _dp_gather(self):
        hdist.allgather_rows_(self.feat_all, self.m.tap('align.tv'))      # [that | vhat] rows as the forward left them: no copy

    def _dp_part_b(self, opts):
        m, B, fa = self.m, self.shape[0], self.feat_all
        lib.check(self._lib.hual_align_loss_rows(
            lib.ptr(fa), ctypes.c_void_p(fa.data_ptr() + 128 * 4), 256, fa.shape[0], hdist.rank() * B if self.world > 1 else 0, B,
            lib.ptr(self.align_scratch), lib.ptr(m.tap('d.align.that')), lib.ptr(m.tap('d.align.vhat')), lib.ptr(self.align_loss),
            float(self.world), lib.stream_ptr()))
        self._backward(opts)

    def _dp_reduce(self):
        hdist.allreduce_sum_(self.m.grads)

    def _dp_part_c(self):
        self._adam(1.0 / self.world)

    def _enqueue_dp(self, drop_rate):
        """one data-parallel step, enqueued without any host synchronisation: forward -> all-gather of the [B,256] alignment
        features -> global [Bg,Bg] alignment loss, gradient rows of the own samples written straight into the backward's
        workspace buffers -> backward -> ONE all-reduce of the flat gradient bucket -> clip + AdamWD on the averaged gradient"""
        opts = self._opts(drop_rate, 1)
        self._dp_part_a(opts)
        self._dp_gather()
        self._dp_part_b(opts)
        self._dp_reduce()
        self._dp_part_c()

    # ------------------------------------------------------------------ capture
    def _warm_up(self, enqueue):
        """one eager step outside capture (first-use hipFuncSetAttribute etc., RCCL channel setup) on a snapshot of the training
        state: the first replay of the graph captured next is the first real step"""
        m = self.m
        state = (m.params, m.adam_m, m.adam_v, m.rng_state) + ((m.ema, m.ema_count) if m.ema is not None else ())
        snap = [t.clone() for t in state]
        enqueue()
        torch.cuda.synchronize()
        for t, s in zip(state, snap):
            t.copy_(s)
        torch.cuda.synchronize()

    def _capture(self, enqueue):
        """Record the launches of `enqueue` as a hipGraph on a side stream, by hand (records, executes nothing).  Not the
        `torch.cuda.graph` context: it synchronises the device and runs the garbage collector on entry - tens of milliseconds per
        shape (our launches allocate nothing, so its private memory pool is not needed either).  A capture costs ~1 ms of host time
        (measured over 250 shapes of the ActivityNet length distribution, scripts/exp/epoch_real.py).
        Returns (graph, None), or (None, error) if the runtime refused the capture.  An error of one of our own launches (lib.HualError:
        bad arguments) would fail eagerly too and is raised, as is anything that is not a RuntimeError."""
        if self._cap_stream is None:
            self._cap_stream = torch.cuda.Stream(device=self.m.device)
        cs, cur = self._cap_stream, torch.cuda.current_stream()
        g = torch.cuda.CUDAGraph()
        cs.wait_stream(cur)
        err = None
        with torch.cuda.stream(cs):
            # thread_local: a capture must not make other threads' HIP calls illegal (a loader thread that synchronises its own stream,
            # the process group's watchdog thread - they would fail AND invalidate the capture in the default global mode); the
            # capturing thread itself only launches kernels
            g.capture_begin(capture_error_mode='thread_local')
            try:
                enqueue()
            except BaseException as ex:          # our own launch failed under capture: end the capture, keep THIS error
                err = ex
            try:
                g.capture_end()
            except RuntimeError as ex:           # the runtime refused the capture
                err = err or ex
        cur.wait_stream(cs)
        if err is None:
            return g, None
        if isinstance(err, lib.HualError) or not isinstance(err, RuntimeError):
            raise err
        return None, err

    def _capture_dp_segments(self, drop_rate):
        """The three runs of OUR launches as three hipGraphs; the collectives stay OUTSIDE and are issued eagerly between the replays -
        no RCCL call inside a graph (that form, _capture_dp_collective, has never run on two devices and stays opt-in), but 57 of the
        step's 59 host launches collapse into three.  Ranks need not agree on it: a rank on segment graphs and a rank on eager
        launches issue the same two collectives in the same order.  Returns None if a capture is refused."""
        opts = self._opts(drop_rate, 1)
        segs = []
        for part in (lambda: self._dp_part_a(opts), lambda: self._dp_part_b(opts), self._dp_part_c):
            g, err = self._capture(part)
            if g is None:
                print('[hual] data-parallel step: segment capture refused (%s) - eager launches' % str(err).splitlines()[0], file=sys.stderr)
                return None
            segs.append(g)
        return segs

    def _capture_dp_collective(self, drop_rate):
        """The data-parallel step WITH its RCCL collectives as ONE hipGraph (nccl backend: its collectives are stream operations).
        The second capture site of this file: torch / RCCL calls run under this capture, so it keeps `torch.cuda.graph` (device
        synchronised on entry, private memory pool) instead of _capture, and the graph-or-eager decision is COLLECTIVE: after the
        attempt the ranks all-reduce(MIN) an ok flag, so either every rank replays or every rank launches eagerly.  Only a refused
        capture (a RuntimeError from torch / HIP) is treated as "no graph" (returns None); an error raised by one of our own launches
        (lib.HualError) propagates."""
        g, err, fatal = None, None, None
        try:
            g = torch.cuda.CUDAGraph()
            # thread_local: the process group's watchdog thread may touch the device while this thread captures
            with torch.cuda.graph(g, capture_error_mode='thread_local'):
                self._enqueue_dp(drop_rate)
        except lib.HualError as e:               # one of our launches failed: not a capture refusal - but the peers are about to
            g, fatal = None, e                   # enter the collective below, so it is raised only after this rank has joined it
        except RuntimeError as e:                # capture of the collectives refused
            g, err = None, e
            torch.cuda.synchronize()
        except BaseException as e:               # anything else: same rule - join the collective first
            g, fatal = None, e
        # the same decision on every rank: 2 = captured, 1 = capture refused (eager launches), 0 = a launch failed (everybody raises)
        state = hdist.global_min(2 if g is not None else (0 if fatal is not None else 1))
        if fatal is not None:
            raise fatal
        if state == 0:
            raise lib.HualError('data-parallel step: a launch failed on another rank during graph capture')
        if state == 1:
            print('[hual] data-parallel step: graph capture %s - eager launches on every rank'
                  % ('refused here (%s)' % str(err).splitlines()[0] if err is not None else 'refused on another rank'), file=sys.stderr)
            return None
        return g

    def _dp_mode(self):
        """HUAL_DP_GRAPH: '1' = the whole step incl. its RCCL collectives as ONE hipGraph (default on a one-rank group: the rehearsal the
        GPU suite runs; opt-in with more ranks - never validated on two devices), 'seg' = three graphs of our own launches
        with the two collectives eager between them (default with more than one rank; a rank whose capture is refused simply launches
        eagerly), '0' = eager launches.  Measured on a one-rank RCCL group: eager 1.253 ms/step, one graph with the collectives inside
        1.210, the single-GPU graph 1.195."""
        return os.environ.get('HUAL_DP_GRAPH', '1' if self.world == 1 else 'seg')

    def _launcher_kind(self):
        """what a step may be captured as: 'graph' (single GPU: the whole step), 'seg' / 'collective' (data parallel, _dp_mode),
        None (eager launches only)"""
        if not self.dp:
            return 'graph' if self.use_graph else None
        if not self.dp_graph:
            return None
        mode = self._dp_mode()
        if mode == 'seg':
            return 'seg'
        # collectives inside a graph: static batches only, and only where they are stream operations (gloo: host collectives)
        if mode == '1' and not self.dynamic and hdist.backend() == 'nccl':
            return 'collective'
        return None

    def _record(self, kind, enqueue, drop_rate):
        """the step's launches as a launcher of `kind`; None, after a line on stderr, if the runtime refused the capture"""
        if kind == 'seg':
            return self._capture_dp_segments(drop_rate)
        if kind == 'collective':
            return self._capture_dp_collective(drop_rate)
        g, err = self._capture(lambda: enqueue(drop_rate))
        if g is None:
            if not self.dynamic:
                raise err
            print('[hual] step graph capture refused for shape %s (%s): eager launches' % (self.shape[:4], str(err).splitlines()[0]),
                  file=sys.stderr)
        return g

    def _replay(self, s):
        g = s.graph
        if type(g) is list:
            g[0].replay()
            self._dp_gather()
            g[1].replay()
            self._dp_reduce()
            g[2].replay()
        else:
            g.replay()
        s.tables_ready = True     # (a graph recorded before the job table was written holds the launches that write it)

    def step(self, lr, drop_rate):
        m = self.m
        if m.lr_value != float(lr):               # the fed scalar changes once per epoch (main.py:61): no fill launch otherwise
            m.lr.fill_(float(lr))
            m.lr_value = float(lr)
        self._launch(self._enqueue_dp if self.dp else self._enqueue_single, self._launcher_kind(), drop_rate)
        m.global_step += 1

    def _launch(self, enqueue, kind, drop_rate):
        """Replay the current step if it is captured for this drop rate; else capture it if it may be (kind, no earlier refusal) and
        is due, and replay - nothing executes while recording, the replay IS the step; else launch eagerly.
        The two modes differ in when a step is due.  A static step (set_batch) is due at once and is warmed up first.  A device-fed
        one (set_batch_device) is due after `capture_after` eager sightings of its (shape, addresses) key, which are its warm-up (first-use
        attribute calls happen outside any capture); `stats` counts these steps only."""
        s, dyn = self._cur, self.dynamic
        how = 'replayed'
        if s.graph is None or s.drop != drop_rate:
            how = 'eager'
            if kind is not None and not s.nograph and (s.seen >= self.capture_after or not dyn):
                if not dyn:
                    self._warm_up(lambda: enqueue(drop_rate))
                g = self._record(kind, enqueue, drop_rate)
                if g is not None:
                    s.graph, s.drop, how = g, drop_rate, 'captured'
                else:                             # refused: this step stays on eager launches for good
                    s.nograph = True
                    if dyn:
                        self.stats['capture_failed'] += 1
        if how == 'eager':
            enqueue(drop_rate)
            s.seen += 1
        else:
            self._replay(s)
        if dyn:
            self.stats[how] += 1
        if self.dp:
            self.dp_launch = 'eager' if how == 'eager' else _DP_LAUNCH[type(s.graph) is list]

    # ------------------------------------------------------------------ one epoch on a device-resident training set
    def run_epoch(self, dataset, order, batch_size, lr, drop_rate, min_chars=4, want_spans=True):
        """The loop of runner_utils.py:139-159 (train_epoch) on a DeviceDataset: for every batch of `order` (sample ids, already
        shuffled - data_loader.py:23-28) assemble the feeds on the device, run the train step, bank the predicted spans.

        Nothing in the loop waits for the device and nothing is uploaded per step: the permutation goes up ONCE, a batch's ids
        are a slice of it; the feeds are views of one set of max-shape buffers; the workspace and the fetch tensors are sized
        once; a step is one hipGraph launch for every padded shape seen before (set_batch_device); the spans of each step are
        copied (device to device, by the NEXT step's assembly launch) into an epoch-long bank that is fetched with ONE transfer after
        the last step - the reference's IoU bookkeeping (runner_utils.py:150-156) only needs them at the end of the epoch.

        Data parallel (world > 1; `batch_size` = clips per rank): every rank calls this with the SAME dataset and order.  A global
        batch is batch_size * world consecutive ids, rank r trains on its r-th slice, padded to the GLOBAL batch's (T, L, C); the
        matching-loss denominator comes from the global batch's lengths on the host; plan: hual_amd/dist.py shard_plan (the < world
        clips that do not fill the last round are dropped from the epoch).  The spans of all ranks are gathered once, after the
        last step.

        Returns (start, end) int64 numpy arrays for the ids of `self.last_epoch_ids` (= `order` unless clips were dropped), in that
        order - (None, None) with want_spans False."""
        m = self.m
        order = np.ascontiguousarray(order, dtype=np.int32)
        world, rank = (self.world, hdist.rank()) if self.world > 1 else (1, 0)
        if world > 1:
            hdist.check_same(int(np.dot(order.astype(np.int64) % 1000003, np.arange(1, len(order) + 1) % 1009) % (1 << 40)) + len(order),
                             "the epoch's sample order")
        steps, dropped = hdist.shard_plan(order, batch_size, world, dataset.vlen_h, dataset.nwords_h, dataset.maxchars_h, min_chars)
        nsteps, bs = len(steps), int(batch_size)
        self.last_epoch_ids = np.concatenate([st['ids'] for st in steps]) if steps else order[:0]
        self.stats['dropped'] = self.stats.get('dropped', 0) + dropped
        if nsteps == 0:
            return (order[:0].astype(np.int64),) * 2 if want_spans else (None, None)
        Bmax = max(st['B'] for st in steps)
        if self._feed_owner is not dataset or self._feeds['shape'][0] < Bmax:
            self._feeds = dataset.feed_buffers(Bmax, min_chars=min_chars)
            self._feed_owner = dataset
        Bm, Tm, Lm, Cm = self._feeds['shape']
        self.reserve(Bm, Tm, Lm, Cm)
        # the ids this rank trains on, step after step, uploaded ONCE; the epoch's position is a device cursor that the step's own
        # last launch advances (hual_adamw_clip_step_loop), and the step's first launch is its batch assembly at that position
        # (hual_assemble_batch_cursor): a step of a known padded shape is ONE graph launch and nothing else - no eager launch between
        # two step graphs (each cost ~10 us of idle device on either side), nothing uploaded, nothing fetched
        mine = np.concatenate([st['ids'][rank * st['B']:(rank + 1) * st['B']] for st in steps])
        lp = self._ensure_loop(dataset, len(mine), nsteps)
        lp['ids'][:len(mine)].copy_(torch.from_numpy(np.ascontiguousarray(mine)))
        lp['cursor'].zero_()
        self._loop = lp
        t_host = time.perf_counter()
        try:
            for st in steps:
                T, L, C = st['shape']
                lp['views'] = dataset.feed_views(st['B'], T, L, C, self._feeds)
                self._host_denom = (st['frames'] + 1e-12) / world if self.dp else None
                self.set_batch_device(lp['views'])
                self.step(lr=lr, drop_rate=drop_rate)
        finally:
            self._host_denom = None
            self._loop = None
        self.stats['host_enqueue_s'] = self.stats.get('host_enqueue_s', 0.0) + (time.perf_counter() - t_host)
        if not want_spans:
            return None, None
        Bcap = self.spans.shape[1]
        bank = lp['bank'][:nsteps * 2 * Bcap].view(nsteps, 2, Bcap)
        host = hdist.allgather_cat(bank).cpu().numpy() if world > 1 else bank.cpu().numpy()[None]      # the epoch's only device -> host transfer
        st_, en_ = [], []
        for i, stp in enumerate(steps):
            for r in range(world):
                st_.append(host[r, i, 0, :stp['B']])
                en_.append(host[r, i, 1, :stp['B']])
        return np.concatenate(st_), np.concatenate(en_)

    def _ensure_loop(self, dataset, n_ids, nsteps):
        """device state of the epoch loop: the rank's id list, the cursor {ids consumed, bank words written} and the span bank
        [steps, 2, B capacity].  Allocated once per (dataset size, fetch capacity) - the step graphs hold these addresses."""
        lp = self._loop_state
        Bcap = self.spans.shape[1]
        if lp is None or lp['ds'] is not dataset or lp['ids'].numel() < n_ids or lp['bank'].numel() < nsteps * 2 * Bcap or lp['Bcap'] != Bcap:
            dev = self.m.device
            # capacity for ANY epoch over this set (a batch size of one: as many steps as samples; 34 MB for ActivityNet at B 64), so
            # that a later epoch with another batch size or order never moves the buffers
            cap = max(n_ids, nsteps, len(dataset), 1)
            lp = dict(ds=dataset, Bcap=Bcap, ids=torch.zeros(cap, dtype=torch.int32, device=dev),
                      cursor=torch.zeros(2, dtype=torch.int64, device=dev),
                      bank=torch.zeros(cap * 2 * Bcap, dtype=torch.int64, device=dev), views=None)
            self._loop_state = lp
        return lp

    def last_loss(self):
        """total loss of the last step (device sync).  DP: local loc/match terms + the global alignment loss."""
        l = self.loss_terms[0]
        if self.dp:
            l = l + self.align_loss[0]
        return l
