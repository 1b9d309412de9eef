"""Thin driver with the loop contract of /root/reference/main.py:50-111 and utils/runner_utils.py:139-176 on the HIP path.

    reference                                               here
    ----------------------------------------------------    -------------------------------------------------------
    main.py --mode train   (epochs, lr decay :61, best       Runner.train(epochs) -> per-epoch "TRAIN:\\t..\\nTEST:\\t.."
      R1@0.7 checkpoint :71-75)                               lines, best checkpoint = <ckpt_dir>/best_SeqPAN.npz
    main.py --mode test                                      Runner.test()
    main.py --mode infer_trainset -> results/<task>/<suffix>.pkl   Runner.infer_trainset(path)
    runner_utils.train_epoch / test_epoch (IoU bookkeeping)  Runner.train_epoch / Runner.test_epoch
    tf.train.Saver                                           numpy .npz keyed by the TF variable names
    (neither has)                                            train.ema_decay: evaluation and best-epoch selection on averaged weights;
                                                             Runner.save_state / load_state / train(resume=...): a run split across visits

Data: the records the reference's dataset_gen leaves (utils/data_gen.py:98-125: vid, duration, v_len, words, w_ids, c_ids,
s_ind, e_ind) + {vid: float32 [n, vdim]} features; both go to HBM once (hual_amd/dataset.py).  Python `random` is seeded here
(the reference leaves the epoch order unseeded).  There is no CPU fallback.
"""
import contextlib
import logging
import os
import pickle
import random
import time

import numpy as np
import torch

from . import al, data, lib
from . import dist as hdist
from .dataset import DeviceDataset
from .model import SeqPAN
from .params import WORD_TABLE

STATE_FORMAT = 1      # Runner.save_state
from .train import Trainer


def _packed(n, groups, dev):
    """one byte buffer on dev that holds, block after block, an [n, columns] array ([n] with columns None) for each (dtype, columns) of
    groups - the widest dtype first, so that every block is aligned -> (its typed views, host): host() copies the buffer in ONE
    transfer and gives the same views of the copy as numpy arrays"""
    ends = np.cumsum([dt.itemsize * n * (c or 1) for dt, c in groups]).tolist()
    assert all(a % dt.itemsize == 0 for (dt, _), a in zip(groups, [0] + ends)), 'a block of %s is not aligned: widest dtype first' % (groups,)

    def views(buf):
        return tuple(buf[a:b].view(dt).view((n, c) if c else (n,)) for (dt, c), a, b in zip(groups, [0] + ends, ends))
    buf = torch.empty(ends[-1], dtype=torch.uint8, device=dev)
    return views(buf), lambda: tuple(x.numpy() for x in views(buf.cpu()))


class Runner:
    def __init__(self, configs, word_vectors, train_records, test_records, visual_feats, device='cuda:0', seed=12345,
                 ckpt_dir=None, logger=None, feed='device'):
        """configs: dict with the keys of configs/<task>/SeqPAN.yaml (+ num_chars, num_words like main.py:35-36).
        feed='host': the training features stay in host memory and every batch is padded on the host and uploaded through the pinned
        pipeline of hual_amd/feeder.py (the reference's own data path, for feature sets beyond the HBM); default: the training set
        lives in HBM and batches are assembled there."""
        assert feed in ('device', 'host')
        self.configs = configs
        self.feed = feed
        self._host_train = (train_records, visual_feats) if feed == 'host' else None
        self._feeder = None
        # (same parameter seed on every rank of a data-parallel job, its own dropout stream per rank)
        self.model = SeqPAN(configs, word_vectors, device=device, seed=seed, rng_seed=seed + 1000003 * hdist.rank())
        self.train_set = DeviceDataset(train_records, visual_feats, device=device) if feed == 'device' else None
        self.test_set = DeviceDataset(test_records, visual_feats, device=device) if test_records else None
        self.batch_size = int(configs['train']['batch_size'])
        self.droprate = float(configs['train']['droprate'])
        self.lr = float(configs['train']['lr'])
        self.ckpt_dir = ckpt_dir or os.path.join('ckpt', '%s_' % configs.get('task', 'task'))      # main.py:42 (sic)
        self.log = logger or logging.getLogger('hual_amd')
        self.rand = random.Random(seed)
        # data parallel when torch.distributed is initialised (one process per GPU, every rank constructs the same Runner with the
        # same seed): configs.train.batch_size is then the batch PER RANK, the global batch is world times that
        self.world, self.rank = hdist.world_size(), hdist.rank()
        self.trainer = Trainer(self.model, world=self.world, use_graph=True)     # per-shape step graphs (Trainer.set_batch_device)
        self.clips_per_s = 0.0
        # where train() stands: the next epoch, the epoch count its lr schedule runs over (main.py:61), the best R1@0.7 so far and
        # its log lines - part of save_state
        self.progress = dict(epoch=0, epochs=int(configs['train'].get('epochs', 1)), best=-1.0, best_lines=None)

    def _weights(self, weights):
        """context of an evaluation pass: the averaged weights by default where the model keeps them (train.ema_decay), else the raw ones"""
        if self.model.ema is None:
            if weights not in (None, 'raw'):
                raise lib.HualError("weights=%r: this run keeps no averaged weights (train.ema_decay is absent or 0)" % (weights,))
            return contextlib.nullcontext()
        return self.model.use_weights(weights or 'ema')

    # ------------------------------------------------------------------ runner_utils.train_epoch (:139-159)
    @staticmethod
    def _ious(records, sidx, eidx):
        return al.ious_of_spans(records, sidx, eidx)

    def _train_epoch_host(self, cur_lr):
        """runner_utils.train_epoch with the reference's own data path: process_batch on the host (hual_amd/data.py), one upload per
        step behind the previous step (hual_amd/feeder.py)"""
        from .feeder import HostFeeder
        recs, feats = self._host_train
        if self.world > 1:
            raise lib.HualError('feed=\'host\' is single-process: the data-parallel loop shards the device-resident set (Trainer.run_epoch)')
        N, bs = len(recs), self.batch_size
        if self._feeder is None:
            T = max(int(r['v_len']) for r in recs)
            L = max(len(r['w_ids']) for r in recs)
            C = max(4, max(len(w) for r in recs for w in r['c_ids']))
            self._feeder = HostFeeder(self.trainer, capacity=(min(bs, N), T, L, C), vdim=int(next(iter(feats.values())).shape[1]))
        order = list(range(N))
        self.rand.shuffle(order)                                   # data_loader.py:24

        t0 = time.perf_counter()
        # every batch is padded straight into a pinned slot (HostFeeder.feed_records: process_batch without the intermediate arrays; words
        # padded to >= 4 characters - the char CNN's widest filter, modules.py:19-38) while the device runs the previous step
        for lo in range(0, N, bs):
            self._feeder.feed_records([recs[i] for i in order[lo:lo + bs]], feats, cur_lr, self.droprate, min_chars=4)
        spans = self._feeder.collect()
        self.clips_per_s = N / max(time.perf_counter() - t0, 1e-9)
        st = np.concatenate([s for s, _ in spans])
        en = np.concatenate([e for _, e in spans])
        if (st < 0).any() or not np.isfinite(float(self.trainer.last_loss())):
            raise lib.HualError('training diverged out of the split-fp16 operand range: %d clip(s) of this epoch came back with span -1 '
                                '(loss %s).  Lower the learning rate or clip_norm; the last good checkpoint is %s'
                                % (int((st < 0).sum()), float(self.trainer.last_loss()), os.path.join(self.ckpt_dir, 'best_SeqPAN.npz')))
        return al.iou_metrics(self._ious([recs[i] for i in order], st, en))

    def set_soft_labels(self, y1, y2, w):
        """soft start / end labels for the training set (DeviceDataset.set_soft_labels): the following epochs train on them"""
        if self.feed == 'host':
            raise ValueError("feed='host' builds the reference's labels on the host: soft labels need the device-resident set (feed='device')")
        self.train_set.set_soft_labels(y1, y2, w)

    def train_epoch(self, cur_lr):
        if self.feed == 'host':
            return self._train_epoch_host(cur_lr)
        ds, N = self.train_set, len(self.train_set)
        order = list(range(N))
        self.rand.shuffle(order)                                   # data_loader.py:24
        t0 = time.perf_counter()
        # the whole epoch is enqueued without a host wait; the spans come back in one transfer (Trainer.run_epoch)
        st, en = self.trainer.run_epoch(ds, order, self.batch_size, lr=cur_lr, drop_rate=self.droprate, min_chars=4)
        self.clips_per_s = N / max(time.perf_counter() - t0, 1e-9)
        # spans of -1 are the kernels' overflow marker (include/hual_seqpan.h: a weight beyond the scaled fp16 image's range, |w| >= 63, or
        # an activation beyond the fp16 operand range, |x| >= 4094, turned a clip's logits into NaN): the float32 reference would still
        # be finite there, so the run stops and says so instead of training on
        if (np.asarray(st) < 0).any() or not np.isfinite(float(self.trainer.last_loss())):
            bad = int((np.asarray(st) < 0).sum())
            raise lib.HualError('training diverged out of the split-fp16 operand range: %d clip(s) of this epoch came back with span -1 '
                                '(loss %s).  Lower the learning rate or clip_norm; the last good checkpoint is %s'
                                % (bad, float(self.trainer.last_loss()), os.path.join(self.ckpt_dir, 'best_SeqPAN.npz')))
        ious = self._ious([ds.records[i] for i in self.trainer.last_epoch_ids], st, en)       # (= order unless world > 1 dropped a tail)
        return al.iou_metrics(ious)

    # ------------------------------------------------------------------ runner_utils.test_epoch (:161-176)
    def test_epoch(self, dataset=None, weights=None):
        """weights: 'ema' (the default with train.ema_decay) or 'raw'"""
        with self._weights(weights):
            return self._test_epoch(dataset)

    def _test_epoch(self, dataset):
        ds = dataset or self.test_set
        ious = []
        for k, lo in enumerate(range(0, len(ds), self.batch_size)):
            if k % self.world != self.rank:                        # batches dealt round-robin to the ranks, IoUs gathered below
                continue
            sel = np.arange(lo, min(len(ds), lo + self.batch_size))
            f = ds.assemble(sel, labels=False, min_chars=4)
            o = self.model.forward(f['video'], f['video_seq_len'], f['word_ids'], f['char_ids'], drop_rate=0.0)
            ious += self._ious([ds.records[i] for i in sel], o['start_index'].cpu().numpy(), o['end_index'].cpu().numpy())
        if self.world > 1:
            parts = hdist.gather_objects(ious)
            ious = hdist.broadcast_object([x for p in parts for x in p] if self.rank == 0 else None)
        return al.iou_metrics(ious)

    # ------------------------------------------------------------------ R@k evaluation (top-k proposals after temporal NMS)
    BAYES_IOUS = (0.3, 0.5, 0.7)      # the thresholds of the reported R@1 (al.iou_metrics): one Bayes span each

    def evaluate(self, dataset=None, k=5, nms_iou=0.5, max_len=0, return_proposals=False, weights=None, rerank=None, hit_iou=0.7,
                 bayes_spans=False, bayes_sets=False):
        """weights: 'ema' (the default with train.ema_decay) or 'raw'; everything else: _evaluate"""
        if rerank not in (None, 'expected_iou', 'hit_prob'):
            raise ValueError("rerank: None, 'expected_iou' or 'hit_prob'")
        thr = lib.hit_thresholds((hit_iou,)) if rerank == 'hit_prob' else None      # (raises on a threshold the kernel cannot take)
        with self._weights(weights):
            return self._evaluate(dataset, k, nms_iou, max_len, return_proposals, rerank, hit_iou, thr, bayes_spans, bayes_sets)

    def _evaluate(self, dataset, k, nms_iou, max_len, return_proposals, rerank=None, hit_iou=0.7, hit_thr=None, bayes_spans=False, bayes_sets=False):
        """R1 and R<k> at IoU 0.3 / 0.5 / 0.7 and mIoU (percent) of the k best spans per clip after greedy temporal NMS
        (hual_span_topk).  Batches and ranks as test_epoch; the proposals of all batches collect on the device and come back in one
        transfer.  R1 and mIoU are those of the first proposal, which is the span test_epoch scores.  return_proposals: also a list
        with one entry per clip of the dataset, [(start_sec, end_sec, score), ...] best first (data.index_to_time).
        rerank='expected_iou': the k proposals of every clip are re-ordered by their expected temporal IoU under the clip's span
        distribution, best first (hual_span_expected_iou with reorder, one more launch per batch into the same buffers) - the
        minimum-Bayes-risk choice among them.  R1 and mIoU are then those of the re-ranked first proposal (R<k> does not depend on the
        order); the result gains 'conf', the mean expected IoU of the first proposal, and 'span_entropy', the mean entropy of the span
        distribution in bits (clips without a value - a poisoned row - count out), and the proposal tuples a fourth element, the
        expected IoU.
        rerank='hit_prob': the same with the proposals' hit probability at IoU >= hit_iou, P(IoU(span, truth) >= hit_iou) under the
        clip's span distribution (hual_span_hit_prob, one more launch per batch, reordering by that threshold's column) - among the
        proposals the choice that maximises the chance of an R1@hit_iou hit.  The result gains 'hit_conf', the mean hit probability of
        the first proposal, and 'ece@<hit_iou>' / 'brier@<hit_iou>', the expected calibration error and the Brier score of that
        probability against the first proposal's actual hit (al.hit_calibration of it and al.topk_ious >= hit_iou); the proposal
        tuples gain the hit probability as a fourth element.
        bayes_spans=True (with any rerank): one more launch per batch finds, for each of IoU 0.3 / 0.5 / 0.7, the span of maximal hit
        probability over ALL spans of the clip, not only the proposals; the result gains 'R1_bayes@0.3' / '@0.5' / '@0.7', the R@1 of
        each threshold's own span at that threshold (through al.ious_of_spans), and 'bayes_conf@...', their mean hit probability.
        bayes_sets=True (with any rerank or bayes_spans): one more launch per batch (hual_span_hit_cover, K = k at IoU 0.3 / 0.5 / 0.7)
        gives the coverage of the proposals - the chance under the clip's span distribution that at least one of them hits, what R<k>
        counts - and per threshold the greedy set of k spans over ALL spans of the clip that covers the most.  The result gains
        'R<k>_bayes@m', the R@k of each threshold's greedy set at that threshold (al.recall_at_k, the rule of 'R<k>@m'),
        'bayes_set_conf@m', the mean coverage of those sets, 'set_conf@m', the mean coverage of the k proposals scored, and
        'set_ece@m' / 'set_brier@m', the calibration of that coverage against whether the clip counted for R<k>@m
        (al.hit_calibration)."""
        ds = dataset or self.test_set
        N, bs, k = len(ds), self.batch_size, int(k)
        mine = [(lo, min(N, lo + bs)) for b, lo in enumerate(range(0, N, bs)) if b % self.world == self.rank]
        n = sum(hi - lo for lo, hi in mine)
        dev = self.model.device
        # one buffer for the three outputs: starts | ends (int64) | scores (float32), each [n,k]
        (st, en, sc), top_host = _packed(n, ((torch.int64, k), (torch.int64, k), (torch.float32, k)), dev)
        # re-ranking: expected IoU [n,k] | span entropy [n] (float32), one more buffer
        (cei, cent), conf_host = _packed(n, ((torch.float32, k), (torch.float32, None)), dev) if rerank == 'expected_iou' else ((None, None), None)
        # hit probability [n,k,1] of the one threshold; the Bayes spans: starts | ends (int64) | probabilities (float32), each [n,3]
        hbuf = torch.empty(n, k, 1, dtype=torch.float32, device=dev) if rerank == 'hit_prob' else None
        (bst, ben, bpr), bayes_host = _packed(n, ((torch.int64, 3), (torch.int64, 3), (torch.float32, 3)), dev) if bayes_spans else ((None,) * 3, None)
        # the sets: greedy starts | ends (int64, [n,3,k]) | their coverage | the proposals' coverage [n,k,3] (float32)
        (cst, cen, cpr, spr), sets_host = (_packed(n, ((torch.int64, 3 * k), (torch.int64, 3 * k), (torch.float32, 3 * k), (torch.float32, 3 * k)), dev)
                                           if bayes_sets else ((None,) * 4, None))
        pos = 0
        for lo, hi in mine:
            sel = np.arange(lo, hi)
            rows = slice(pos, pos + hi - lo)
            f = ds.assemble(sel, labels=False, min_chars=4)
            o = self.model.forward(f['video'], f['video_seq_len'], f['word_ids'], f['char_ids'], drop_rate=0.0)
            lib.span_topk(o['start_logits'], o['end_logits'], f['video_seq_len'], k, max_len=max_len, nms_iou=nms_iou,
                          out=(st[rows], en[rows], sc[rows]))
            if rerank == 'expected_iou':
                lib.span_expected_iou(o['start_logits'], o['end_logits'], f['video_seq_len'], st[rows], en[rows], score=sc[rows], reorder=True,
                                      out=(cei[rows], cent[rows]))
            if rerank == 'hit_prob':
                lib.span_hit_prob(o['start_logits'], o['end_logits'], f['video_seq_len'], hit_thr, st[rows], en[rows], score=sc[rows],
                                  reorder_by=0, out=(hbuf[rows], None))
            if bayes_spans:
                lib.span_hit_prob(o['start_logits'], o['end_logits'], f['video_seq_len'], self.BAYES_IOUS, best=True,
                                  out=(None, (bst[rows], ben[rows], bpr[rows])))
            if bayes_sets:
                lib.span_hit_cover(o['start_logits'], o['end_logits'], f['video_seq_len'], self.BAYES_IOUS, st[rows], en[rows], K=k,
                                   out=(spr[rows].view(-1, k, 3), tuple(x[rows].view(-1, 3, k) for x in (cst, cen, cpr))))
            pos += hi - lo
        ids = np.concatenate([np.arange(lo, hi) for lo, hi in mine]) if mine else np.zeros(0, dtype=np.int64)
        part = (ids,) + top_host()
        if rerank == 'expected_iou':
            part += conf_host()
        if rerank == 'hit_prob':
            part += (hbuf.cpu().numpy().reshape(n, k),)
        if bayes_spans:
            part += bayes_host()
        if bayes_sets:
            part += sets_host()
        if self.world > 1:
            parts = hdist.gather_objects(part)
            if self.rank == 0:
                part = tuple(np.concatenate([p[x] for p in parts]) for x in range(len(part)))
            part = hdist.broadcast_object(part if self.rank == 0 else None)
        ids, S, E, SC = part[:4]
        recs = [ds.records[i] for i in ids]
        ious = al.topk_ious(recs, S, E)
        r1 = al.iou_metrics(ious[:, 0])
        rk = al.recall_at_k(recs, S, E)
        res = {'R1@0.3': r1[0], 'R1@0.5': r1[1], 'R1@0.7': r1[2], 'R%d@0.3' % k: rk[0], 'R%d@0.5' % k: rk[1], 'R%d@0.7' % k: rk[2],
               'mIoU': r1[3]}
        self.log.info('EVAL (k={}, nms_iou={}):\tR1 {:.2f}\t{:.2f}\t{:.2f}\tR{} {:.2f}\t{:.2f}\t{:.2f}\tmIoU {:.2f}'.format(
            k, nms_iou, r1[0], r1[1], r1[2], k, rk[0], rk[1], rk[2], r1[3]))
        if rerank == 'expected_iou':
            EI, ENT = part[4], part[5]
            c0, ent = EI[:, 0][EI[:, 0] >= 0], ENT[ENT >= 0]
            res['conf'] = float(np.mean(c0, dtype=np.float64)) if c0.size else float('nan')
            res['span_entropy'] = float(np.mean(ent, dtype=np.float64)) if ent.size else float('nan')
            self.log.info('EVAL re-ranked by expected IoU:\tconf {:.4f}\tspan entropy {:.3f} bits'.format(res['conf'], res['span_entropy']))
        if rerank == 'hit_prob':
            EI = part[4]                                           # (the proposals' fourth element below)
            h0 = EI[:, 0][EI[:, 0] >= 0]
            cal = al.hit_calibration(EI[:, 0], ious[:, 0] >= hit_iou)
            res['hit_conf'] = float(np.mean(h0, dtype=np.float64)) if h0.size else float('nan')
            res['ece@%g' % hit_iou], res['brier@%g' % hit_iou] = cal['ece'], cal['brier']
            self.log.info('EVAL re-ranked by hit probability at IoU {:g}:\thit conf {:.4f}\tECE {:.4f}\tBrier {:.4f}'.format(
                hit_iou, res['hit_conf'], cal['ece'], cal['brier']))
        if bayes_spans:
            BS, BE, BP = part[-7:-4] if bayes_sets else part[-3:]
            for c, m in enumerate(self.BAYES_IOUS):
                hit = al.topk_ious(recs, BS[:, c], BE[:, c])[:, 0] >= m      # (a clip without a span - a poisoned row - is a miss)
                bp = BP[:, c][BP[:, c] >= 0]
                res['R1_bayes@%g' % m] = float(np.mean(hit) * 100.0)
                res['bayes_conf@%g' % m] = float(np.mean(bp, dtype=np.float64)) if bp.size else float('nan')
            self.log.info('EVAL Bayes spans (maximal hit probability per threshold):\tR1 ' + '\t'.join(
                '{:.2f}'.format(res['R1_bayes@%g' % m]) for m in self.BAYES_IOUS))
        if bayes_sets:
            CS, CE, CP = (x.reshape(len(ids), 3, k) for x in part[-4:-1])
            SP = part[-1].reshape(len(ids), k, 3)
            counted = ious.max(axis=1, initial=0.0)                # (the clip counts for R<k>@m iff this is >= m: al.recall_at_k)
            for c, m in enumerate(self.BAYES_IOUS):
                cp, sp = CP[:, c, k - 1][CP[:, c, k - 1] >= 0], SP[:, k - 1, c][SP[:, k - 1, c] >= 0]
                cal = al.hit_calibration(SP[:, k - 1, c], counted >= m)
                res['R%d_bayes@%g' % (k, m)] = al.recall_at_k(recs, CS[:, c], CE[:, c], thresholds=(m,))[0]
                res['bayes_set_conf@%g' % m] = float(np.mean(cp, dtype=np.float64)) if cp.size else float('nan')
                res['set_conf@%g' % m] = float(np.mean(sp, dtype=np.float64)) if sp.size else float('nan')
                res['set_ece@%g' % m], res['set_brier@%g' % m] = cal['ece'], cal['brier']
            self.log.info('EVAL Bayes sets (greedy maximal coverage per threshold):\tR{} '.format(k) + '\t'.join(
                '{:.2f}'.format(res['R%d_bayes@%g' % (k, m)]) for m in self.BAYES_IOUS) + '\tset conf ' + '\t'.join(
                '{:.4f}'.format(res['set_conf@%g' % m]) for m in self.BAYES_IOUS))
        if not return_proposals:
            return res
        props = [None] * N
        for row, i in enumerate(ids):
            r, p = ds.records[i], []
            for c, (s, e, x) in enumerate(zip(S[row], E[row], SC[row])):
                if s >= 0:
                    t0, t1 = data.index_to_time((s, e), r['v_len'], r['duration'])
                    p.append((float(t0), float(t1), float(x)) + ((float(EI[row, c]),) if rerank else ()))
            props[i] = p
        return res, props

    # ------------------------------------------------------------------ main.py --mode train (:50-78)
    def cur_lr(self):
        """the learning rate of the next epoch (main.py:61)"""
        pr = self.progress
        return self.lr * (1.0 - pr['epoch'] / pr['epochs'])

    def run_one_epoch(self, state_path=None):
        """the body of main.py's epoch loop at self.progress: train, test, keep the best R1@0.7 (on the averaged weights where the run
        keeps them), move on; with state_path, rank 0 then writes the training state"""
        pr = self.progress
        self.log.info('Epoch {}|{}:'.format(pr['epoch'], pr['epochs']))
        r = self.train_epoch(self.cur_lr())
        train_line = 'TRAIN:\t{:.2f}\t{:.2f}\t{:.2f}\t{:.2f}\t'.format(*r)
        self.log.info(train_line + '({:.0f} clips/s)'.format(self.clips_per_s))
        test_line = ''
        r1i7 = r[2]
        if self.test_set is not None:
            t = self.test_epoch()
            test_line = 'TEST:\t{:.2f}\t{:.2f}\t{:.2f}\t{:.2f}\t'.format(*t)
            self.log.info(test_line)
            r1i7 = t[2]
        if r1i7 > pr['best']:                                     # main.py:71-75
            pr['best'] = r1i7
            if self.rank == 0:
                self.save(os.path.join(self.ckpt_dir, 'best_SeqPAN.npz'))
            pr['best_lines'] = '\n' + train_line + '\n' + test_line
        pr['epoch'] += 1
        if state_path is not None and self.rank == 0:
            self.save_state(state_path)

    def train(self, epochs=None, resume=None, state_path=None):
        """resume: a file of save_state to continue from (read by every rank); state_path: where rank 0 writes the state after every
        epoch (may be the same file)"""
        pr = self.progress
        if resume is not None:
            self.load_state(resume)
            if epochs is not None and int(epochs) != pr['epochs']:
                raise lib.HualError('%s was written by a run over %d epochs: continuing it over %d would change the learning rate '
                                    'schedule' % (resume, pr['epochs'], int(epochs)))
        else:
            pr.update(epoch=0, epochs=int(epochs if epochs is not None else self.configs['train']['epochs']), best=-1.0, best_lines=None)
        while pr['epoch'] < pr['epochs']:
            self.run_one_epoch(state_path)
        self.log.info('\n\nHighest R1i7 epoch\n')
        self.log.info(pr['best_lines'])
        return pr['best']

    def test(self):
        hdist.barrier()                                            # rank 0 wrote the checkpoint
        self.load(os.path.join(self.ckpt_dir, 'best_SeqPAN.npz'))
        t = self.test_epoch()
        self.log.info('TEST:\t{:.2f}\t{:.2f}\t{:.2f}\t{:.2f}\t'.format(*t))
        return t

    # ------------------------------------------------------------------ main.py --mode infer_trainset (:99-111)
    def infer_trainset(self, path=None, mc_dropout=None, load_best=True, weights=None, mc_samples=None, mc_stat='range', bank=None,
                       span_conf=False, grad_bank=None, grad_hyp='prediction'):
        """results/<task>/<suffix>.pkl of runner_utils.py:103-104.  mc_dropout=None: as the reference runs.
        weights: 'ema' (the default with train.ema_decay) or 'raw'.  mc_samples=K (with mc_dropout): K stochastic passes folded into
        `bank` (al.McBank; default: one of this call only) - the records then hold 'prop_uncert' instead of prop_logits1/2: the statistic
        mc_stat = 'range' or 'std', or 'bald', 'entropy' or 'expected_entropy' (a given bank was then built with info=True).
        span_conf=True: the records also hold 'prop_conf' and 'prop_span_entropy' (al.infer_trainset).
        grad_bank: an al.GradBank over the training set - the pass fills it with the gradient embeddings of the span heads under the
        hypothesis grad_hyp, and the records also hold 'prop_egl' and 'prop_gnorm2' (al.infer_trainset; single process only)."""
        if load_best:
            hdist.barrier()
            self.load(os.path.join(self.ckpt_dir, 'best_SeqPAN.npz'))
        if self.train_set is None:          # feed='host': the inference pass works on a device-resident set, built on first use
            self.train_set = DeviceDataset(*self._host_train, device=self.model.device)
        with self._weights(weights):
            records, ious = al.infer_trainset_sharded(self.model, self.train_set, self.batch_size, mc_dropout=mc_dropout, min_chars=4,
                                                      mc_samples=mc_samples, bank=bank, mc_stat=mc_stat, span_conf=span_conf,
                                                      **({} if grad_bank is None else dict(grad_bank=grad_bank, grad_hyp=grad_hyp)))
        if self.rank != 0:
            return None, hdist.broadcast_object(None)
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, 'wb') as f:
                pickle.dump(records, f)
        m = hdist.broadcast_object(al.iou_metrics(ious))
        self.log.info('predict train set:\t{:.2f}\t{:.2f}\t{:.2f}\t{:.2f}\t'.format(*m))
        return records, m

    # ------------------------------------------------------------------ checkpoints by TF variable name
    def save(self, path):
        """the parameters by TF variable name; a run with averaged weights adds <name>/ExponentialMovingAverage for every variable
        (TensorFlow's own naming) and the update count"""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        named = self.model.state_dict()
        if self.model.ema is not None:
            named.update(self.model.ema_state_dict())
        np.savez(path, **{k.replace('/', '|'): v for k, v in named.items()})

    def load(self, path):
        with np.load(path) as z:
            named = {k.replace('|', '/'): z[k] for k in z.files}
        if self.model.finetune_word_emb and WORD_TABLE not in named:
            self.log.info('%s holds no %s: fine-tuning starts from the GloVe table' % (path, WORD_TABLE))
        self.model.load_state_dict(named)

    # ------------------------------------------------------------------ the whole training state: a run continued on another visit
    def save_state(self, path):
        """Everything that determines how the run goes on: parameters, Adam moments, averaged weights and their count, the Philox
        state, the step count, train()'s position and best epoch, and the shuffle stream.  Written under a temporary name and renamed
        into place: a kill during the write leaves the previous file whole."""
        m, pr = self.model, self.progress
        ver, words, gauss = self.rand.getstate()
        d = dict(format=np.int64(STATE_FORMAT), flat_floats=np.int64(m.params.numel()), params=m.params.cpu().numpy(),
                 adam_m=m.adam_m.cpu().numpy(), adam_v=m.adam_v.cpu().numpy(), rng_state=m.rng_state.cpu().numpy(),
                 global_step=np.int64(m.global_step), epoch=np.int64(pr['epoch']), epochs=np.int64(pr['epochs']),
                 best=np.float64(pr['best']), best_lines=np.array('' if pr['best_lines'] is None else pr['best_lines']),
                 has_best=np.int64(pr['best_lines'] is not None), rand_version=np.int64(ver),
                 rand_words=np.array(words, dtype=np.uint64), rand_gauss=np.float64(np.nan if gauss is None else gauss),
                 ema_decay=np.float64(m.ema_decay))
        if m.ema is not None:
            d.update(ema=m.ema.cpu().numpy(), ema_count=m.ema_count.cpu().numpy())
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tmp = '%s.tmp.%d' % (path, os.getpid())
        try:
            with open(tmp, 'wb') as f:
                np.savez(f, **d)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)

    def load_state(self, path):
        """the inverse of save_state, on every rank (ranks other than 0 keep the seed words of their own dropout stream and take its
        offset).  The file and the run must agree on whether averaged weights are kept."""
        m, pr = self.model, self.progress
        with np.load(path) as z:
            d = {k: z[k] for k in z.files}
        if int(d.get('format', -1)) != STATE_FORMAT:
            raise lib.HualError('%s is not a training state of this version (Runner.save_state)' % path)
        if ('ema' in d) != (m.ema is not None):
            raise lib.HualError('%s was written %s averaged weights and this run is configured %s them: set train.ema_decay %s'
                                % ((path, 'with', 'without', 'to %g to continue it' % float(d['ema_decay'])) if 'ema' in d else
                                   (path, 'without', 'with', 'to 0 (or drop it) to continue it')))
        if int(d['flat_floats']) != m.params.numel():
            raise lib.HualError('%s holds %d parameters, this model %d: another model configuration' % (path, int(d['flat_floats']), m.params.numel()))
        dev = m.device
        for name in ('params', 'adam_m', 'adam_v') + (('ema', 'ema_count') if m.ema is not None else ()):
            getattr(m, name).copy_(torch.from_numpy(d[name]).to(dev))
        rs = torch.from_numpy(d['rng_state']).to(dev)
        if self.rank == 0:
            m.rng_state.copy_(rs)
        else:
            m.rng_state[2:].copy_(rs[2:])
        m.global_step = int(d['global_step'])
        pr.update(epoch=int(d['epoch']), epochs=int(d['epochs']), best=float(d['best']),
                  best_lines=str(d['best_lines']) if int(d['has_best']) else None)
        g = float(d['rand_gauss'])
        self.rand.setstate((int(d['rand_version']), tuple(int(x) for x in d['rand_words']), None if np.isnan(g) else g))
