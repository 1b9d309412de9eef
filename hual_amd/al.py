"""Active-learning round pieces around the SeqPAN hot path, MI355X side.

    reference                                                    here
    ---------------------------------------------------------    -------------------------------------------------
    runner_utils.eval_test_save (utils/runner_utils.py:69-110)   infer_trainset(model, batches): ONE deterministic
      five sess.run per batch + results/<task>/<suffix>.pkl        forward (all five fetches) + two stochastic forwards
    update_label.main (update_label.py:173-208)                  update_labels(data_old, data_gt, last_prop, coff):
      python loop over samples, sorted() inside the loop           two launches over the whole training set
    update_label.get_coff / F_renew (update_label.py:11-37,212)  get_coff / F_RENEW

The scoring and the pseudo-label re-derivation run in libhual_seqpan.so (csrc/al.hip, through hual_al_score /
hual_al_renew); ranking, ground-truth lookup (the "annotator") and time<->index conversion are a few numpy lines on the
host.  There is no CPU fallback: without the library or a GPU this module raises.

Reference quirk kept selectable: eval-mode get_feed_dict (runner_utils.py:61-65) drops drop_rate, so the
reference's two "dropout 0.5" passes run WITHOUT dropout and prop_logits1 == prop_logits2 == prop_logits;
mc_dropout=None reproduces that, mc_dropout=0.5 is what the code intends.

K-pass uncertainty (neither has): infer_trainset(mc_dropout=0.5, mc_samples=K, bank=McBank) runs K >= 2 stochastic forwards per batch
and folds each into a device-resident bank of per-frame statistics (hual_al_mc_fold); no stochastic logit reaches the host, the records
carry 'prop_uncert' instead of 'prop_logits1/2', and LabelUpdater.from_bank / update_labels(bank=) score straight from the bank
(hual_al_score_mc).  Without mc_samples every launch, record and result is what it was.

Information-theoretic acquisition (neither has): mc_stat 'bald', 'entropy' or 'expected_entropy' instead of 'range' / 'std' - the
mutual information between prediction and dropout mask, the entropy of the mean prediction and the mean entropy of the passes, in bits,
summed over the two heads: each in [0, 2] at every K.  They need a McBank built with info=True, whose folds (hual_al_mc_fold_info) also
keep the running mean of the per-pass entropy, and are scored by hual_al_score_info.  Without those names every launch, record and
result is what it was.

Span confidence (neither has): infer_trainset(span_conf=True) adds to every record the expected temporal IoU of its own proposal under
the deterministic pass's span distribution ('prop_conf', in [0, 1]) and that distribution's entropy in bits ('prop_span_entropy') - one
hual_span_expected_iou launch per batch, fetched with the deterministic fetches.  update_labels(rank_by='span_risk') then selects the
half of the set with the smallest risk 1 - prop_conf instead of the smallest uncert_video.  Off by default: every launch, record and
result is then what it was.

The question by expected information gain (neither has): update_labels(observe_by='info_gain') asks every selected sample about the
frame whose answer says most about the span - the argmax of h2(q(t)), q(t) the probability that t lies inside the span under the span
distribution of the deterministic pass restricted to the spans the earlier answers allow (LabelUpdater.query, one hual_al_query launch
over the whole set) - instead of the argmax of uncert_frame.  Off by default: every launch, record and result is then what it was.

The pseudo-label by minimum Bayes risk (neither has): update_labels(renew_by='posterior') gives every selected sample, instead of
renew_label's hand-tuned mix (F_RENEW), the span of maximal expected temporal IoU under that same posterior - restricted to the spans
the answers allow, this round's included - with that expectation as its confidence (LabelUpdater.mbr_label, one hual_al_mbr_label
launch over the selected samples; a sample whose answers contradict each other or whose row is poisoned keeps the reference's renew,
one hual_al_renew launch over just those).  Off by default: every launch, record and result is then what it was.

Acquisition by expected label gain (neither has): update_labels(acquire_by='label_gain') chooses both the samples that are asked and
the frame each is asked about by the temporal IoU the minimum-Bayes-risk label is expected to gain from the answer - one-step lookahead
under that same posterior, in the evaluation's own metric (LabelUpdater.label_gain, one hual_al_label_gain launch over the whole set):
the half of the set with the largest gain is selected, each sample asked at its frame of maximal gain (the reference's frame where no
answer can move the label).  Off by default: every launch, record and result is then what it was.

Training on the posterior (neither has): run_round(soft_labels=lam) trains the round's epochs not on the three-frame kernel around the
hard pseudo-label alone but, for every sample with an answer, on its blend (weight lam) with the start and end marginals of that same
posterior, this round's answers included (LabelUpdater.span_marginals, one hual_al_span_marginals launch over the whole set;
update_labels(soft_out=) hands them out; DeviceDataset.set_soft_labels feeds them to the assembly launch).  Off by default: every
launch, record and result is then what it was.

An annotator who errs (the reference simulates a perfect one): update_labels(answer_noise=eps) reads all of the above from the span
posterior under answers that are wrong with probability eps - the product form of logits tilted by the answers (LabelUpdater.tilt, one
hual_al_noisy_tilt launch; the gain by hual_al_label_gain_noisy), on which no answer is a hard constraint and no sample contradictory;
annotator_flip=(rate, rng) simulates such an annotator.  Off by default: every launch, record and result is then what it was.

Calibration (all of the above take the model's softmaxes at face value and eps from the caller): update_labels(calibrate='evidence')
first fits a temperature tau and the error rate eps to the answers of the earlier rounds by their evidence, the sum over the clips of
ln P(answers | softmax(logits / tau), eps) (LabelUpdater.calibrate: hual_al_evidence_grid on a coarse grid and two zooms), and the
round's posterior readers use the fitted pair (LabelUpdater.set_temperature; temperature= hands one in).  Off by default: every launch,
record and result is then what it was.

Question sets (an annotator who is not in the loop - a labelling tool, a crowd batch, one viewing of a clip - takes the frames of a
clip together): update_labels(questions_at_once=M) asks every selected sample about the M frames of most JOINT information under its
span posterior, the greedy design of the entropy of their answer vector (LabelUpdater.design, one hual_al_design launch for all of
them), and answers them on the host.  Off by default: every launch, record and result is then what it was.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import lib

# update_label.py:11-37 (index = active-learning round I; entry 0 unused)
F_RENEW = {
    'charades': {'pos': {'old': [None, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], 'model': [None, 0.8, 0.8, 0.8, 0.8, 0.8, 0.8],
                         'distance': [None, 4.0, 0.2, 0.2, 0.2, 0.2, 0.2]},
                 'neg': {'old': [None, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], 'model': [None, 2.4, 0.2, 0.2, 0.2, 0.2, 0.2],
                         'distance': [None, 2.0, 0.2, 0.2, 0.2, 0.2, 0.2]},
                 'uncert': [None, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25]},
    'anet': {'pos': {'old': [None, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], 'model': [None, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0],
                     'distance': [None, 2.0, 1.8, 1.6, 1.5, 1.5, 1.5]},
             'neg': {'old': [None, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], 'model': [None, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0],
                     'distance': [None, 2.0, 1.8, 1.6, 1.5, 1.5, 1.5]},
             'uncert': [None, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25]},
}


def get_coff(task, I):
    """(pos.distance, pos.model, pos.old, neg.distance, neg.model, neg.old, uncert) of round I (update_label.py:212-218)"""
    t = F_RENEW[task]
    return (t['pos']['distance'][I], t['pos']['model'][I], t['pos']['old'][I],
            t['neg']['distance'][I], t['neg']['model'][I], t['neg']['old'][I], t['uncert'][I])


# ---------------------------------------------------------------- K-pass uncertainty bank ---------
STAT_NAMES = "the statistic is 'range' or 'std', or - from a McBank with info=True - 'bald', 'entropy' or 'expected_entropy'"


def check_passes(passes):
    """McBank's passes argument -> Kmax, 0 for None; raises ValueError"""
    if passes is None:
        return 0
    try:
        ok = not isinstance(passes, bool) and int(passes) == passes and 1 <= int(passes) <= lib.AL_ENS_MAX_K
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('McBank: passes is None or an integer in [1, %d]' % lib.AL_ENS_MAX_K)
    return int(passes)


def check_part_passes(part, Kmax):
    """the rows of McBank.export_rows against the bank that imports them: both keep the passes, as many, or neither does"""
    have = int(part['pass_s'].shape[0]) if 'pass_s' in part else 0
    if have != Kmax:
        raise lib.HualError('McBank.import_rows: the rows keep passes=%s and the bank passes=%s - build both banks with the same passes='
                            % (have or None, Kmax or None))


class McBank:
    """Per-sample statistics of K stochastic forwards over a training set of N samples, resident on the device (hual_al_bank):
    tlen i32 [N]; the deterministic logits s0 / e0 f32 [N, ld]; per head (0 = start, 1 = end) the minimum, maximum, Welford mean and
    sum of squared deviations of the per-frame probabilities, stats f32 [2, 4, N, ld] = [head, (lo, hi, mean, m2)].
    K: the number of stochastic passes folded so far (the largest k seen since the last k = 1).
    info=True adds ent f32 [2, N, ld] (hual_al_info): per head the running mean of the passes' binary entropy h2(p_k) in bits, folded by
    the same launch (hual_al_mc_fold_info) - what the statistics 'bald', 'entropy' and 'expected_entropy' are read from.
    passes=Kmax (1..16; None: no such buffer, every launch and bit as without the argument) keeps the passes themselves beside their
    statistics: pass_s / pass_e f32 [Kmax, N, ld], plane k - 1 the raw logits of stochastic pass k - what the span posterior's model
    average reads (hual_al_ensemble_query / hual_al_ensemble_label, LabelUpdater.set_ensemble)."""
    FIELDS = ('lo', 'hi', 'mean', 'm2')

    def __init__(self, N, ld, device='cuda:0', info=False, passes=None):
        if not torch.cuda.is_available():
            raise lib.HualError('McBank needs a GPU: the HIP path has no CPU fallback')
        if N < 1 or not 2 <= ld <= 1024:
            raise ValueError('McBank: need N >= 1 and 2 <= ld <= 1024')
        self._lib = lib.load()
        self.dev = torch.device(device)
        self.N, self.ld, self.K = int(N), int(ld), 0
        self.tlen = torch.zeros(N, dtype=torch.int32, device=self.dev)
        self.s0 = torch.zeros(N, ld, device=self.dev)
        self.e0 = torch.zeros(N, ld, device=self.dev)
        self.stats = torch.zeros(2, 4, N, ld, device=self.dev)
        self.ent = torch.zeros(2, N, ld, device=self.dev) if info else None
        self.Kmax = check_passes(passes)
        self.pass_s = torch.zeros(self.Kmax, N, ld, device=self.dev) if self.Kmax else None
        self.pass_e = torch.zeros(self.Kmax, N, ld, device=self.dev) if self.Kmax else None
        self._bind()

    @classmethod
    def for_dataset(cls, dataset, device='cuda:0', info=False, passes=None):
        """a bank over a DeviceDataset: one row per sample, as wide as its longest clip"""
        return cls(len(dataset), max(2, int(np.max(dataset.vlen_h))), device=device, info=info, passes=passes)

    def _bind(self):
        a, st = lib._addr, self.stats
        self.c = lib.hual_al_bank(self.N, self.ld, a(self.tlen), a(self.s0), a(self.e0), a(st[0, 0]), a(st[0, 1]), a(st[0, 2]), a(st[0, 3]),
                                  a(st[1, 0]), a(st[1, 1]), a(st[1, 2]), a(st[1, 3]))
        self.info_c = lib.hual_al_info(a(self.ent[0]), a(self.ent[1])) if self.ent is not None else None

    def stat(self, head, name):
        """[N, ld] view: head 0 = start / 1 = end, name in ('lo', 'hi', 'mean', 'm2'), and 'ent' on a bank with info=True"""
        if name == 'ent':
            self.need_info('ent')
            return self.ent[head]
        return self.stats[head, self.FIELDS.index(name)]

    def need_info(self, what):
        if self.ent is None:
            raise lib.HualError("McBank: '%s' needs the passes' entropy, which this bank does not fold - build the bank with info=True" % what)

    def check_stat(self, stat):
        """raises unless this bank can be read as the statistic `stat`"""
        if stat in lib.AL_STAT_INFO:
            self.need_info(stat)
        elif stat not in lib.AL_STAT:
            raise ValueError('stat: ' + STAT_NAMES)

    def rows(self, ids):
        """device i32 row ids of one fold, checked on the host: inside the bank, none twice (the rows of a launch must be disjoint)"""
        ids = np.ascontiguousarray(ids.cpu().numpy() if torch.is_tensor(ids) else ids, dtype=np.int64).reshape(-1)
        if ids.size == 0 or ids.min() < 0 or ids.max() >= self.N:
            raise lib.HualError('McBank.fold: row ids must lie in [0, %d)' % self.N)
        if np.unique(ids).size != ids.size:
            raise lib.HualError('McBank.fold: a row id is repeated - the rows of one fold must be disjoint')
        return torch.from_numpy(ids.astype(np.int32)).to(self.dev)

    def fold(self, ids, v_len, start_logits, end_logits, k, _checked=False):
        """one forward's logits f32 [B, T_b] (device) into the rows `ids` (host array, list or tensor); k = 0: the deterministic pass,
        k = 1..K: the stochastic ones, in order.  Enqueued on the current stream.  A bank with passes=Kmax also keeps the logits of
        pass k >= 1 in plane k - 1 (rows ids, columns [0, T_b)); k > Kmax raises before anything is folded."""
        if self.pass_s is not None and int(k) > self.Kmax:
            raise lib.HualError('McBank.fold: pass %d of a bank that keeps passes=%d' % (int(k), self.Kmax))
        if not _checked:
            ids = self.rows(ids)
        s, e = start_logits, end_logits
        if s.dtype != torch.float32 or e.dtype != torch.float32 or s.dim() != 2 or e.shape != s.shape:
            raise lib.HualError('McBank.fold: start / end logits must both be float32 [B, T_b]')
        s, e = s.contiguous(), e.contiguous()
        B, T = s.shape
        vl = v_len.to(device=self.dev, dtype=torch.int32).contiguous()
        if ids.numel() != B or vl.numel() != B:
            raise lib.HualError('McBank.fold: ids and v_len must hold B = %d entries' % B)
        if self.ent is not None:
            lib.check(self._lib.hual_al_mc_fold_info(ctypes.byref(self.c), ctypes.byref(self.info_c), lib.ptr(ids), lib.ptr(vl), lib.ptr(s),
                                                     lib.ptr(e), B, T, int(k), lib.stream_ptr()))
        else:
            lib.check(self._lib.hual_al_mc_fold(ctypes.byref(self.c), lib.ptr(ids), lib.ptr(vl), lib.ptr(s), lib.ptr(e), B, T, int(k),
                                                lib.stream_ptr()))
        if k >= 1:
            self.K = int(k) if k == 1 else max(self.K, int(k))
            if self.pass_s is not None:                          # (plumbing: one indexed copy per head)
                rows = ids.long()
                self.pass_s[int(k) - 1, rows, :T] = s
                self.pass_e[int(k) - 1, rows, :T] = e

    def uncert(self, K=None, stat='range'):
        """the model-uncertainty term f32 [N, ld] of every frame as hual_al_score_mc ('range', 'std') or hual_al_score_info ('bald',
        'entropy', 'expected_entropy'; a bank with info=True) computes it (by that launch itself, so a value read here is the value a
        later score uses, bit for bit); columns beyond a row's tlen are 0"""
        K = self.K if K is None else int(K)
        self.check_stat(stat)
        N, ld = self.N, self.ld
        tl = self.tlen.cpu().numpy()
        if tl.min() < 0 or tl.max() > ld:
            raise lib.HualError('McBank.uncert: a row length outside [0, ld] - the bank is not initialised')
        z = torch.zeros(N + 1, dtype=torch.int32, device=self.dev)
        one = torch.zeros(1, dtype=torch.int32, device=self.dev)
        aset = lib.hual_al_set(N, ld, lib._addr(self.tlen), lib._addr(self.tlen), lib._addr(z), lib._addr(one),
                               lib._addr(torch.zeros(1, dtype=torch.int8, device=self.dev)))
        um = torch.zeros(N, ld, device=self.dev)
        scratch = torch.empty(2, N, ld, device=self.dev)
        uf = torch.empty(N, ld, device=self.dev, dtype=torch.float64)
        uv = torch.empty(N, device=self.dev)
        ob = torch.empty(N, device=self.dev, dtype=torch.int32)
        lib.al_score(aset, self.s0, self.e0, 0.0, (scratch[0], scratch[1], uf, uv, ob), bank=self.c, info=self.info_c, K=K, stat=stat,
                     uncert_model=um)
        torch.cuda.current_stream().synchronize()          # (the launch's inputs above are locals)
        return um

    # rows as host arrays and back: how the ranks of a sharded pass hand their (disjoint) rows to rank 0 - copied, never reduced
    # ('ent' travels with them when the bank holds it; a part and a bank must agree on that)
    def export_rows(self, ids):
        i = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(self.dev)
        part = dict(ids=np.ascontiguousarray(ids, dtype=np.int64), tlen=self.tlen[i].cpu().numpy(), s0=self.s0[i].cpu().numpy(),
                    e0=self.e0[i].cpu().numpy(), stats=self.stats[:, :, i].cpu().numpy(), K=self.K)
        if self.ent is not None:
            part['ent'] = self.ent[:, i].cpu().numpy()
        if self.pass_s is not None:
            part['pass_s'], part['pass_e'] = self.pass_s[:, i].cpu().numpy(), self.pass_e[:, i].cpu().numpy()
        return part

    def import_rows(self, part):
        if ('ent' in part) != (self.ent is not None):
            raise lib.HualError("McBank.import_rows: the rows %s 'ent' and the bank %s - build both banks with the same info="
                                % (('hold', 'has none') if 'ent' in part else ('lack', 'folds it')))
        check_part_passes(part, self.Kmax)
        if len(part['ids']) == 0:
            return
        i = torch.from_numpy(part['ids']).to(self.dev)
        self.tlen[i] = torch.from_numpy(part['tlen']).to(self.dev)
        self.s0[i] = torch.from_numpy(part['s0']).to(self.dev)
        self.e0[i] = torch.from_numpy(part['e0']).to(self.dev)
        self.stats[:, :, i] = torch.from_numpy(part['stats']).to(self.dev)
        if self.ent is not None:
            self.ent[:, i] = torch.from_numpy(part['ent']).to(self.dev)
        if self.pass_s is not None:
            self.pass_s[:, i] = torch.from_numpy(part['pass_s']).to(self.dev)
            self.pass_e[:, i] = torch.from_numpy(part['pass_e']).to(self.dev)
        self.K = max(self.K, int(part['K']))


def attach_uncert(records, rows, bank, K, stat):
    """records[j]['prop_uncert'] = the model-uncertainty term f32 [T_b] of bank row rows[j], read from the bank once"""
    um = bank.uncert(K, stat).cpu().numpy()
    tl = bank.tlen.cpu().numpy()
    for r, n in zip(records, rows):
        r['prop_uncert'] = um[n, :tl[n]].copy()


# ---------------------------------------------------------------- infer_trainset ----------------
GRAD_HYP = ('prediction', 'pseudo')


class GradBank:
    """the gradient embeddings of a whole training set on the device (hual_al_grad_embed): desc f32 [N, 256] - the gradient of the
    localizing loss with respect to the start_dense / end_dense kernels under a hypothesised span, columns 0..127 g_s and 128..255
    g_e -, gnorm2 f32 [N] its squared length and egl f32 [N] the expected squared gradient length under y ~ p.  infer_trainset(grad_bank=)
    writes the rows of the samples it sees, one launch per batch; a row nobody wrote holds zeros.  desc is the descriptor space of
    badge_select / update_labels(select_by='badge'), egl the scalar of rank_by='egl'."""

    def __init__(self, N, device='cuda:0'):
        N = int(N)
        if N < 1:
            raise ValueError('GradBank: N >= 1')
        self.N, self.device = N, torch.device(device)
        self.desc = torch.zeros(N, lib.GRAD_EMBED_DIM, dtype=torch.float32, device=self.device)
        self.gnorm2 = torch.zeros(N, dtype=torch.float32, device=self.device)
        self.egl = torch.zeros(N, dtype=torch.float32, device=self.device)

    @classmethod
    def for_dataset(cls, dataset, device=None):
        return cls(len(dataset), device=dataset.dev if device is None else device)

    def rows(self, ids):
        """the bank rows of the samples `ids` as the launch reads them: device int32, range-checked here"""
        ids = np.asarray(ids, dtype=np.int64)
        if ids.ndim != 1 or (ids.size and (ids.min() < 0 or ids.max() >= self.N)):
            raise ValueError('GradBank: sample ids outside [0, %d)' % self.N)
        return torch.from_numpy(ids.astype(np.int32)).to(self.device)

    def embed(self, model, out, lens, rows, hyp):
        """one hual_al_grad_embed launch on the label-free forward `model` has just run (`out`: its fetches): reads model.tap('head.hs')
        / ('head.he') in place where the workspace table shows that nothing else lives in their bytes, else copies of them made in the
        forward's stream.  hyp: device int32 [B, 2]."""
        taps, private = _head_taps(model)
        if not private:
            taps = tuple(t.clone() for t in taps)
        return lib.al_grad_embed(taps[0], taps[1], out['start_logits'], out['end_logits'], lens, hyp, self.desc, self.gnorm2, self.egl,
                                 rows=rows)


def _head_taps(model):
    """-> ((head.hs, head.he) views of the workspace, private): private is False when another entry of hual_seqpan_ws_table overlaps
    the bytes of either - a later launch of the same forward could then have overwritten them, and a reader must copy them out in the
    forward's stream.  The table gives every named buffer its own range today, so the views are read in place."""
    table = model._ws_table
    private = True
    for name in ('head.hs', 'head.he'):
        off, rows, cols = table[name]
        end = off + rows * cols * 4
        for other, (o2, r2, c2) in table.items():
            if other != name and o2 < end and off < o2 + r2 * c2 * 4:
                private = False
    return (model.tap('head.hs'), model.tap('head.he')), private


def attach_grad(records, rows, grad_bank):
    """records[j]['prop_egl'] / ['prop_gnorm2'] = the floats of bank row rows[j], read from the bank once"""
    egl, gn = grad_bank.egl.cpu().numpy(), grad_bank.gnorm2.cpu().numpy()
    for r, n in zip(records, rows):
        r['prop_egl'], r['prop_gnorm2'] = float(egl[n]), float(gn[n])


def infer_trainset(model, batches, mc_dropout=None, batch_ids=None, rng=None, mc_samples=None, bank=None, sample_ids=None,
                   mc_stat='range', _attach=True, span_conf=False, grad_bank=None, grad_hyp='prediction'):
    """eval_test_save (runner_utils.py:69-110) without the file write: returns (records, ious).

    batches: iterable of (raw_records, video, video_seq_len, word_ids, char_ids) as TestLoader.test_iter yields them
    (data_loader.py:131-143).  Each record of the result has the keys of runner_utils.py:90-100; logits are the raw
    [T_b] rows of the batch (unmasked beyond v_len), m_score is [T_b, 4].
    batch_ids (with mc_dropout): the position of each yielded batch in the whole pass - the two stochastic forwards of batch i use the
    Philox offsets base + 2 i and base + 2 i + 1, whichever rank runs the batch and whatever ran before it (infer_trainset_sharded);
    rng = (seed, base) of that stream (default: the model's own state).
    mc_samples=K (>= 2, with mc_dropout and a McBank `bank` over the whole set): the deterministic forward plus K stochastic ones, each
    followed by one fold into the bank rows sample_ids[i] (one array of row ids per yielded batch; default: the samples in the order
    they arrive).  Only the five deterministic fetches go to the host.  Pass k of batch i uses the Philox offset base + K i + (k - 1) -
    today's two at K = 2.  The records lose prop_logits1/2 and gain 'prop_uncert' (f32 [T_b], the statistic `mc_stat` = 'range' or
    'std' of hual_al_score_mc, or 'bald', 'entropy' or 'expected_entropy' of hual_al_score_info from a bank with info=True; read from
    the bank once at the end).
    span_conf=True: every record gains 'prop_conf' (float: the expected temporal IoU of its own prop_idx under the span distribution of
    the deterministic pass, -1.0 where the forward gave no span) and 'prop_span_entropy' (float, bits): one hual_span_expected_iou
    launch per batch with k = 1 on the forward's start_index / end_index, fetched with the five deterministic fetches.
    grad_bank: None (every launch and record as without the argument), or a GradBank over the whole set - after the deterministic
    forward of a batch one hual_al_grad_embed launch writes the bank rows sample_ids[i] (default: arrival order) from the forward's
    head.hs / head.he, its logits and the hypothesis grad_hyp: 'prediction' (the forward's own start_index / end_index - BADGE's
    hypothesised label) or 'pseudo' (the records' s_ind / e_ind).  The records gain 'prop_egl' and 'prop_gnorm2' (floats, -1.0 for a
    sample whose logits are not finite), read from the bank once at the end.  Single process only.
    """
    from . import data
    records, ious = [], []
    if grad_hyp not in GRAD_HYP:
        raise ValueError("grad_hyp: 'prediction' or 'pseudo'")
    if grad_bank is not None:
        from . import dist as hdist
        if not isinstance(grad_bank, GradBank):
            raise ValueError('grad_bank: a GradBank over the whole training set')
        if hdist.world_size() > 1:
            raise ValueError('grad_bank is single-process only: the rows of other ranks are not gathered')
    K = None
    if mc_samples is not None:
        K = int(mc_samples)
        if K < 2:
            raise ValueError('mc_samples: K >= 2 stochastic passes (one sample has no spread)')
        if mc_dropout is None:
            raise ValueError('mc_samples needs mc_dropout: K passes without dropout are K copies of one')
        if bank is None:
            raise ValueError('mc_samples needs a McBank (bank=) over the whole training set')
        bank.check_stat(mc_stat)                                # (before K forwards per batch are spent on a bank that cannot answer)
    sample_ids = iter(sample_ids) if sample_ids is not None else None
    rows_seen = []
    batch_ids = iter(batch_ids) if batch_ids is not None else None
    rng_base = rng_seed = None
    if batch_ids is not None and mc_dropout is not None:
        rng_seed, rng_base = (int(rng[0]), int(rng[1])) if rng is not None else model.get_rng()
    P = 0 if mc_dropout is None else 2 if K is None else K      # stochastic passes per batch: folded into the bank, or two kept

    def enqueue(batch):
        """all forwards of a batch (one deterministic + P stochastic), nothing fetched: the device runs them while the host
        writes the records of the batch before"""
        raw, video, lens, word_ids, char_ids = batch
        o = model.forward(video, lens, word_ids, char_ids, drop_rate=0.0)
        dev = [o['start_logits'], o['end_logits'], o['match_scores'], o['start_index'], o['end_index']]
        conf = None
        if span_conf:
            nb = o['start_index'].numel()
            conf = lib.span_expected_iou(o['start_logits'], o['end_logits'], lens, o['start_index'].view(nb, 1), o['end_index'].view(nb, 1))
        if K is not None or grad_bank is not None:
            n0 = sum(len(x) for x in rows_seen)
            ids = np.asarray(next(sample_ids)) if sample_ids is not None else np.arange(n0, n0 + len(raw))
            rows_seen.append(ids)
        if grad_bank is not None:                                # (before the stochastic forwards overwrite the workspace, in stream order)
            if grad_hyp == 'prediction':
                hyp = torch.stack([o['start_index'], o['end_index']], dim=1).to(torch.int32)
            else:
                hyp = torch.tensor([[int(r['s_ind']), int(r['e_ind'])] for r in raw], dtype=torch.int32).to(model.device)
            lens_d = lens if torch.is_tensor(lens) and lens.is_cuda and lens.dtype == torch.int32 else model._to_dev(lens, torch.int32)
            grad_bank.embed(model, o, lens_d, grad_bank.rows(ids), hyp)
        if K is not None:
            rows = bank.rows(ids)
            bank.fold(rows, lens, o['start_logits'], o['end_logits'], 0, _checked=True)
        if P and rng_base is not None:
            model.set_rng(rng_seed, rng_base + P * int(next(batch_ids)))
        for k in range(1, P + 1):
            ok = model.forward(video, lens, word_ids, char_ids, drop_rate=mc_dropout)
            model.rng_state[2] += 1                              # a fresh Philox offset for the next stochastic pass
            if K is not None:
                bank.fold(rows, lens, ok['start_logits'], ok['end_logits'], k, _checked=True)
            else:
                dev += [ok['start_logits'], ok['end_logits']]
        if conf is not None:
            dev += [conf[0], conf[1]]                            # (last: the positions of the fetches above stay)
        # device -> pinned host, asynchronously on the compute stream; the event marks their arrival
        host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in dev]
        for h, t in zip(host, dev):
            h.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return raw, host, ev

    def emit(job):
        raw, host, ev = job
        ev.synchronize()
        # (copies: the records outlive the loop, the pinned staging buffers should not)
        s0, e0, ms, si, ei = (h.numpy().copy() for h in host[:5])
        if K is not None:
            stoch = None                                        # folded on the device: the records carry prop_uncert instead
        elif mc_dropout is None:
            stoch = (s0, e0, s0, e0)                            # as written: drop_rate never reaches the graph (F8)
        else:
            stoch = tuple(h.numpy().copy() for h in host[5:9])
        ious.extend(ious_of_spans(raw, si, ei))
        for i, r in enumerate(raw):
            rec = {'vid': r['vid'], 'duration': r['duration'], 'psuedo_idx': [r['s_ind'], r['e_ind']],
                   'sentence': ' '.join(r['words']), 'v_len': int(r['v_len']),
                   'prop_idx': [int(si[i]), int(ei[i])], 'prop_logits': [s0[i], e0[i]]}
            if stoch is not None:
                s1, e1, s2, e2 = stoch
                rec['prop_logits1'], rec['prop_logits2'] = [s1[i], e1[i]], [s2[i], e2[i]]
            rec['m_score'] = ms[i]
            if span_conf:
                rec['prop_conf'], rec['prop_span_entropy'] = float(host[-2][i, 0]), float(host[-1][i])
            records.append(rec)

    pending = None
    for batch in batches:
        job = enqueue(batch)                                     # batch n is on the device ...
        if pending is not None:
            emit(pending)                                        # ... while the records of batch n - 1 are written
        pending = job
    if pending is not None:
        emit(pending)
    if K is not None and _attach and records:
        attach_uncert(records, np.concatenate(rows_seen), bank, K, mc_stat)
    if grad_bank is not None and records:
        attach_grad(records, np.concatenate(rows_seen), grad_bank)
    return records, ious


def infer_trainset_sharded(model, dataset, batch_size, mc_dropout=None, min_chars=4, mc_samples=None, bank=None, mc_stat='range',
                           span_conf=False, grad_bank=None, grad_hyp='prediction'):
    """infer_trainset over a DeviceDataset in the reference's order (TrainNoSuffleLoader.test_iter, data_loader.py:167-206), the
    batches dealt round-robin to the ranks of the process group (batch i -> rank i % world; every rank holds the whole set):
    rank 0 returns (records, ious) of the WHOLE set in sample order, the other ranks (None, None).  One rank: the plain pass.
    The batches are the single-process ones (own padded shape each), so the records equal a single-process pass; the Philox offsets
    of the stochastic forwards depend on the batch index only.
    mc_samples=K: every rank folds its own batches into its own bank (`bank`; default: a McBank.for_dataset of this call only, with
    info=True when mc_stat is 'bald', 'entropy' or 'expected_entropy'); the
    rows of the other ranks reach rank 0's bank with the records (disjoint rows: copied, never reduced), and rank 0 reads
    'prop_uncert' from the gathered bank.  Every rank's own stream advances by K * n_batches.
    span_conf: as infer_trainset (the two floats travel with the records).
    grad_bank / grad_hyp: as infer_trainset, the rows being the samples' positions in the set; one process only (ValueError under a
    process group of more, like soft labels)."""
    from . import dist as hdist
    world, rank = hdist.world_size(), hdist.rank()
    if grad_bank is not None and world > 1:
        raise ValueError('grad_bank is single-process only: the rows of other ranks are not gathered')
    N = len(dataset)
    los = list(range(0, N, batch_size))
    own = [i for i in range(len(los)) if i % world == rank]

    def batches():
        for i in own:
            sel = np.arange(los[i], min(N, los[i] + batch_size))
            f = dataset.assemble(sel, out=None, labels=False, min_chars=min_chars)
            yield [dataset.records[k] for k in sel], f['video'], f['video_seq_len'], f['word_ids'], f['char_ids']
    own_rng = model.get_rng()
    rng = hdist.broadcast_object(own_rng)                       # rank 0's stream for the stochastic passes: the records do not depend on `world`
    K = int(mc_samples) if mc_samples is not None else None
    own_rows = [np.arange(los[i], min(N, los[i] + batch_size)) for i in own]
    if K is not None and bank is None:
        bank = McBank.for_dataset(dataset, device=model.device, info=mc_stat in lib.AL_STAT_INFO)
    records, ious = infer_trainset(model, batches(), mc_dropout=mc_dropout, batch_ids=own, rng=rng, mc_samples=mc_samples, bank=bank,
                                   sample_ids=own_rows if K is not None or grad_bank is not None else None, mc_stat=mc_stat, _attach=False,
                                   span_conf=span_conf, grad_bank=grad_bank, grad_hyp=grad_hyp)
    # every rank returns to its OWN dropout stream, behind the whole pass
    model.set_rng(own_rng[0], own_rng[1] + ((2 if K is None else K) * len(los) if mc_dropout is not None else 0))
    part = None
    if K is not None and world > 1 and rank != 0:
        part = bank.export_rows(np.concatenate(own_rows) if own_rows else np.zeros(0, dtype=np.int64))
    parts = hdist.gather_objects((own, records, ious, part))
    if parts is None:
        return None, None
    out_r, out_i = [None] * N, [None] * N
    for own_r, recs_r, ious_r, part_r in parts:
        if part_r is not None:
            bank.import_rows(part_r)
        k = 0
        for i in own_r:
            n = min(N, los[i] + batch_size) - los[i]
            out_r[los[i]:los[i] + n] = recs_r[k:k + n]
            out_i[los[i]:los[i] + n] = ious_r[k:k + n]
            k += n
    if K is not None:
        attach_uncert(out_r, np.arange(N), bank, K, mc_stat)
    return out_r, out_i


def calculate_iou(i0, i1):
    """runner_utils.py:34-38"""
    union = (min(i0[0], i1[0]), max(i0[1], i1[1]))
    inter = (max(i0[0], i1[0]), min(i0[1], i1[1]))
    return max(0.0, 1.0 * (inter[1] - inter[0]) / (union[1] - union[0]))


def ious_of_spans(records, sidx, eidx):
    """IoU of the predicted spans against the records' own (s_ind, e_ind), both through index_to_time (data_utils.py:121-128) and
    calculate_iou (runner_utils.py:34-38): the per-sample loop of runner_utils.py:149-156 for a whole list at once, in the reference's
    own arithmetic (float32 unit grid times, float32 ratio).  Equal to the scalar functions element for element
    (tests/test_data_golden.py)."""
    n = len(records)
    if n == 0:
        return []
    f32 = np.float32
    vl = np.array([r['v_len'] for r in records], dtype=f32)
    du = np.array([float(r['duration']) for r in records], dtype=f32)
    gs = np.array([r['s_ind'] for r in records], dtype=np.int64)
    ge = np.array([r['e_ind'] for r in records], dtype=np.int64)
    ps = np.asarray(sidx, dtype=np.int64)[:n]
    pe = np.asarray(eidx, dtype=np.int64)[:n]

    def t0(i):      # s_times[i] = float32(i) * duration / num_units
        return i.astype(f32) * du / vl

    def t1(i):      # e_times[i] = float32(i + 1) * duration / num_units
        return (i + 1).astype(f32) * du / vl
    st, et, g0, g1 = t0(ps), t1(pe), t0(gs), t1(ge)
    union = np.maximum(et, g1) - np.minimum(st, g0)
    inter = np.minimum(et, g1) - np.maximum(st, g0)
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = inter / union
    return np.where(iou > 0, iou, f32(0.0)).tolist()


def iou_metrics(ious):
    """R@1 IoU={0.3,0.5,0.7} and mIoU in percent (runner_utils.py:25-31,106-109)"""
    a = np.asarray(ious, dtype=np.float64)
    return tuple(float(np.mean(a >= t) * 100.0) for t in (0.3, 0.5, 0.7)) + (float(np.mean(a) * 100.0),)


def topk_ious(records, starts, ends):
    """IoU [N,k] (float64 of the float32 values) of every proposal column through ious_of_spans; a -1 slot (no proposal) counts as 0"""
    n = len(records)
    st = np.asarray(starts, dtype=np.int64).reshape(n, -1)
    en = np.asarray(ends, dtype=np.int64).reshape(n, -1)
    out = np.zeros(st.shape, dtype=np.float64)
    for c in range(st.shape[1]):
        pad = (st[:, c] < 0) | (en[:, c] < 0)
        iou = np.asarray(ious_of_spans(records, np.where(pad, 0, st[:, c]), np.where(pad, 0, en[:, c])), dtype=np.float64)
        out[:, c] = np.where(pad, 0.0, iou) if n else iou
    return out


def recall_at_k(records, starts, ends, thresholds=(0.3, 0.5, 0.7)):
    """R@k in percent for each IoU threshold: the share of clips with at least one of its k proposals (starts / ends [N,k] frame
    indices, -1 = none) at IoU >= threshold.  k = 1 is the R@1 of iou_metrics."""
    best = topk_ious(records, starts, ends).max(axis=1, initial=0.0)
    return tuple(float(np.mean(best >= t) * 100.0) for t in thresholds)


def frame_hits(idx_a, idx_b, thresholds):
    """does span a hit span b at IoU >= m? - the integer rule of hual_span_hit_prob and hual_al_hit_label on the host: idx_a / idx_b
    int [n, 2] frame spans (start, end), thresholds as lib.hit_thresholds takes them -> bool [n, M], den * inter >= num * union on
    the half-open frame intervals [start, end + 1).  A row with a span that is none (an index < 0 or start > end) is no hit.  What
    hit_calibration takes beside the launches' probabilities."""
    a = np.asarray(idx_a, dtype=np.int64).reshape(-1, 2)
    b = np.asarray(idx_b, dtype=np.int64).reshape(-1, 2)
    if a.shape != b.shape:
        raise ValueError('frame_hits: idx_a and idx_b must hold the same number of spans')
    thr = lib.hit_thresholds(thresholds)
    ok = (a[:, 0] >= 0) & (a[:, 0] <= a[:, 1]) & (b[:, 0] >= 0) & (b[:, 0] <= b[:, 1])
    inter = np.maximum(0, np.minimum(a[:, 1], b[:, 1]) + 1 - np.maximum(a[:, 0], b[:, 0]))
    union = (a[:, 1] - a[:, 0] + 1) + (b[:, 1] - b[:, 0] + 1) - inter
    return np.stack([ok & (den * inter >= num * union) for num, den in thr], axis=1)


def hit_calibration(prob, hit, bins=10):
    """reliability of predicted hit probabilities against what happened: prob (floats in [0, 1]; an entry < 0 - no value, as
    hual_span_hit_prob gives for an invalid slot or a poisoned row - counts out) and hit (truth values of the same shape) ->
    dict(count int64 [bins], mean_prob, hit_rate float64 [bins] (NaN for an empty bin), ece, brier, n).  The bins are `bins` equal
    widths on [0, 1]: bin q holds q / bins <= prob < (q + 1) / bins, the last one also prob == 1.  ece is the count-weighted mean over
    the bins of |hit_rate - mean_prob| (the expected calibration error), brier the mean of (prob - hit)^2; both NaN without entries.
    Host only, float64."""
    p = np.asarray(prob, dtype=np.float64).ravel()
    h = np.asarray(hit).ravel().astype(bool)
    if p.shape != h.shape:
        raise ValueError('hit_calibration: prob and hit must have the same number of entries')
    bins = int(bins)
    if bins < 1:
        raise ValueError('hit_calibration: bins >= 1')
    keep = p >= 0
    p, h = p[keep], h[keep].astype(np.float64)
    if p.size and p.max() > 1.0:
        raise ValueError('hit_calibration: prob must not exceed 1')
    q = np.minimum((p * bins).astype(np.int64), bins - 1)
    count = np.bincount(q, minlength=bins).astype(np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean_prob = np.bincount(q, weights=p, minlength=bins) / count
        hit_rate = np.bincount(q, weights=h, minlength=bins) / count
    full = count > 0
    n = int(p.size)
    ece = float(np.sum(count[full] * np.abs(hit_rate[full] - mean_prob[full])) / n) if n else float('nan')
    brier = float(np.mean((p - h) ** 2)) if n else float('nan')
    return dict(count=count, mean_prob=mean_prob, hit_rate=hit_rate, ece=ece, brier=brier, n=n)


# ---------------------------------------------------------------- label update -------------------
def _round_half_even_index(t, duration, vlen):
    """time_to_index_v2 (update_label.py:41-48): python round() of t / duration * (vlen - 1)"""
    return round(t / duration * (vlen - 1))


def check_noise(eps):
    """the annotator's error probability as the launches take it: a float32 in (0, 0.5], returned widened to a python float"""
    try:
        e = float(np.float32(eps))
    except (TypeError, ValueError):
        e = float('nan')
    if isinstance(eps, bool) or not 0.0 < e <= 0.5:
        raise ValueError('the answer noise eps must lie in (0, 0.5]')
    return e


CALIB_TAUS = tuple(2.0 ** (k / 4.0) for k in range(-8, 9))      # the coarse grid of LabelUpdater.calibrate: 1/4 .. 4, tau = 1 in the middle
CALIB_EPS = (0.005, 0.01, 0.02, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5)
CALIB_MIN_EPS = 1e-6                                             # where a zoom towards eps = 0 stops


def _zoom_axis(x, i, n, lo, hi):
    """n points, geometric, from x[i - 1] to x[i + 1] of the ascending positive axis x - where x[i] is its first or last point, one
    step of the neighbouring ratio past it -, clamped to [lo, hi] (lo = 0: no clamp below)"""
    x = np.asarray(x, dtype=np.float64)
    step = x[1] / x[0] if i == 0 else x[i] / x[i - 1]
    left = x[i - 1] if i > 0 else x[i] / step
    right = x[i + 1] if i + 1 < x.size else x[i] * (x[i] / x[i - 1])
    left, right = (max(left, lo) if lo > 0 else left), min(right, hi)
    return np.geomspace(left, right, n) if right > left else np.array([left])


def check_bank_planes(bank, K=None):
    """raises unless `bank` keeps the logits of its K (default: bank.K) stochastic passes"""
    K = int(getattr(bank, 'K', 0) if K is None else K)
    if bank is None or getattr(bank, 'pass_s', None) is None:
        raise ValueError("the ensemble posterior needs a McBank that keeps its passes: build the bank with passes=K")
    if not 1 <= K <= bank.Kmax or K > bank.K:
        raise ValueError('the ensemble posterior needs 1 <= mc_samples <= the passes the bank holds (K = %d, passes = %d)' % (bank.K, bank.Kmax))


class LabelUpdater:
    """Device-side state of one update_label round: the logits of the results pkl as [N, ld] matrices, the active
    points as CSR.  score() and renew() are one launch each.
    Bank form (from_bank, or records that hold 'prop_uncert'): the model-uncertainty term comes from a McBank of K folded passes
    (hual_al_score_mc; hual_al_score_info for the statistics 'bald', 'entropy' and 'expected_entropy') instead of the two stochastic
    passes' logits; there is no [6, N, ld] matrix then.
    Whichever way it is built, the updater records its source - logits (the [6, N, ld] matrix or None), bank (the McBank or None), K and
    stat - and the hual_al_bank / hual_al_info that score() hands to lib.al_score."""

    def __init__(self, last_prop, aps, device='cuda:0'):
        if not torch.cuda.is_available():
            raise lib.HualError('LabelUpdater needs a GPU: the HIP path has no CPU fallback')
        self._lib = lib.load()
        self.dev = torch.device(device)
        N = len(last_prop)
        tlen = np.array([len(p['prop_logits'][0]) for p in last_prop], dtype=np.int32)
        vlen = np.array([p['v_len'] for p in last_prop], dtype=np.int32)
        ld = int(tlen.max())
        if int(tlen.min()) < 2 or ld > 1024 or (vlen < 1).any() or (vlen > tlen).any():
            raise ValueError('need 2 <= len(logits) <= 1024 and 1 <= v_len <= len(logits)')
        with_uncert = ['prop_uncert' in p for p in last_prop]
        if any(with_uncert):
            # a round resumed from records of a K-pass inference: the recorded term itself is the whole state.  As the start head's
            # maximum over a minimum of 0 (end head all 0) the RANGE statistic returns it bit for bit: (u - 0) + (0 - 0)
            if not all(with_uncert):
                raise ValueError("some records hold 'prop_uncert' and some do not")
            lg = np.zeros((2, N, ld), dtype=np.float32)
            um = np.zeros((N, ld), dtype=np.float32)
            for n, p in enumerate(last_prop):
                if len(p['prop_uncert']) != tlen[n]:
                    raise ValueError("'prop_uncert' and 'prop_logits' differ in length")
                lg[0, n, :tlen[n]], lg[1, n, :tlen[n]] = p['prop_logits']
                um[n, :tlen[n]] = p['prop_uncert']
            lg_d = torch.from_numpy(lg).to(self.dev)
            self._s0, self._e0 = lg_d[0], lg_d[1]
            self._um, self._zero = torch.from_numpy(um).to(self.dev), torch.zeros(N, ld, device=self.dev)
            a = lib._addr
            self.bank_c = lib.hual_al_bank(N, ld, None, a(self._s0), a(self._e0), a(self._zero), a(self._um), a(self._zero), a(self._zero),
                                           a(self._zero), a(self._zero), a(self._zero), a(self._zero))
            self._source(None, None, 2, 'range')
        else:
            lg = np.zeros((6, N, ld), dtype=np.float32)
            for n, p in enumerate(last_prop):
                for k, key in enumerate(('prop_logits', 'prop_logits1', 'prop_logits2')):
                    lg[2 * k, n, :tlen[n]] = p[key][0]
                    lg[2 * k + 1, n, :tlen[n]] = p[key][1]
            lg_d = torch.from_numpy(lg).to(self.dev)
            self._s0, self._e0, self.bank_c = lg_d[0], lg_d[1], None
            self._source(lg_d, None, 2, None)
        self._finish(N, ld, tlen, vlen, torch.from_numpy(tlen).to(self.dev), aps)

    @classmethod
    def from_bank(cls, bank, vlen, aps, K=None, stat='range', ensemble=False):
        """score straight from a McBank (no upload, no logits matrix).  vlen: host [N] valid frames; K: the stochastic passes the bank
        holds (default: bank.K); stat: 'range' or 'std' (hual_al_score_mc), or 'bald', 'entropy' or 'expected_entropy' (hual_al_score_info;
        the bank was built with info=True).  ensemble=True: the span posterior's launches read the model average over the bank's K
        kept passes (set_ensemble on its planes; the bank was built with passes >= K)."""
        bank.check_stat(stat)
        if ensemble:
            check_bank_planes(bank, K)
        self = cls.__new__(cls)
        self._lib = lib.load()
        self.dev = bank.dev
        tlen = bank.tlen.cpu().numpy()
        vlen = np.ascontiguousarray(vlen, dtype=np.int32)
        if len(vlen) != bank.N or int(tlen.min()) < 2 or int(tlen.max()) > bank.ld or (vlen < 1).any() or (vlen > tlen).any():
            raise ValueError('need one v_len per bank row, every row folded (tlen >= 2) and 1 <= v_len <= tlen')
        self._s0, self._e0, self.bank_c = bank.s0, bank.e0, bank.c
        self._source(None, bank, int(bank.K if K is None else K), stat)
        if self.K < (1 if stat in ('entropy', 'expected_entropy') else 2):
            if ensemble and self.K == 1:
                raise ValueError("the ensemble posterior itself runs on K = 1 pass, but the round's score reads the statistic '%s', which "
                                 "needs two: use 'entropy' or 'expected_entropy' (a bank with info=True), or K >= 2" % stat)
            raise ValueError('the bank holds K = %d stochastic passes: a spread needs two' % self.K)
        self._finish(bank.N, bank.ld, tlen, vlen, bank.tlen, aps)
        if ensemble:
            self.set_ensemble(bank.pass_s[:self.K], bank.pass_e[:self.K])
        return self

    def _source(self, logits, bank, K, stat):
        """where score() reads the model-uncertainty term from: the stochastic rows of `logits`, or self.bank_c as `stat` over K passes"""
        self.logits, self.bank, self.K, self.stat = logits, bank, K, stat

    def _finish(self, N, ld, tlen, vlen, tlen_d, aps):
        self.N, self.ld = N, ld
        self.tlen_h, self.vlen_h = tlen, vlen
        self.tlen = tlen_d
        self.vlen = torch.from_numpy(vlen).to(self.dev)
        self.sprob = torch.zeros(N, ld, device=self.dev)
        self.eprob = torch.zeros(N, ld, device=self.dev)
        self.uncert_frame = torch.zeros(N, ld, device=self.dev, dtype=torch.float64)
        self.uncert_video = torch.zeros(N, device=self.dev)
        self.observe = torch.zeros(N, device=self.dev, dtype=torch.int32)
        self.temperature, self._inv_tau, self._last_eps = None, None, None
        self._det, self._chain = (self._s0, self._e0), {}        # (the deterministic logits: the chain's source unless it holds another)
        self.set_active_points(aps)

    def set_active_points(self, aps):
        """aps: per sample (list of (frame, is_pos)) in annotation order"""
        self.aps = aps                                           # (the caller's lists, by reference: session() reads them)
        off = np.zeros(self.N + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(a) for a in aps])
        idx = np.array([f for a in aps for f, _ in a] + [0], dtype=np.int32)      # never empty: a valid pointer
        pos = np.array([1 if p else 0 for a in aps for _, p in a] + [0], dtype=np.int8)
        self.ap_off = torch.from_numpy(off).to(self.dev)
        self.ap_idx = torch.from_numpy(idx).to(self.dev)
        self.ap_pos = torch.from_numpy(pos).to(self.dev)
        p = lib.ptr
        self.set = lib.hual_al_set(self.N, self.ld, p(self.vlen).value, p(self.tlen).value, p(self.ap_off).value,
                                   p(self.ap_idx).value, p(self.ap_pos).value)
        self._drop('tilted')                                     # (a tilt holds the answers it was made with)

    # What a launch of the span posterior reads is the last stage of one chain: 'source' - an ensemble's passes [K, N, ld]; without
    # an entry the deterministic logits [N, ld] - -> 'scaled' by float32(1 / tau) -> 'tilted' by the answers under eps.  The two
    # later stages are made on demand and kept in _chain beside what they were made from; _drop is the one place that forgets.
    # One slot per stage: tilt() and _logits() always work on the deterministic logits, so beside an ensemble they and the
    # ensemble's readers take the 'scaled' and 'tilted' slots from each other, and each remakes what it finds made from other rows.
    CHAIN = ('source', 'scaled', 'tilted')

    def _posterior_source(self):
        return self._chain.get('source', self._det)

    def _drop(self, stage):
        """forget `stage` of the chain and every stage made from it"""
        for name in self.CHAIN[self.CHAIN.index(stage):]:
            self._chain.pop(name, None)
        self.tilt_eps = None

    def set_temperature(self, tau):
        """the temperature of the span posterior: None or 1.0 (the default) - the posterior's launches, tilt and session read the
        source's logits themselves, the very same memory, so every launch and stored bit is what it is without this call -, or
        tau > 0: they read s0 * float32(1 / tau) and e0 * float32(1 / tau), one float32 product per logit (the row
        hual_al_evidence_grid evaluates at that tau), computed once and kept until the temperature or the source changes.  score() and renew() restate the
        reference's heuristic and keep reading the unscaled logits.  calibrate() fits tau."""
        if tau is not None:
            try:
                tau = float('nan') if isinstance(tau, bool) else float(tau)
            except (TypeError, ValueError):
                tau = float('nan')
            if not 0.0 < tau < float('inf'):
                raise ValueError('the temperature must be None or a finite number > 0')
        inv = None if tau is None or tau == 1.0 else np.float32(1.0 / tau)
        if inv is not None and not 0.0 < float(inv) < float('inf'):
            raise ValueError('the temperature must be None or a finite number > 0')
        if inv != self._inv_tau:
            self._drop('scaled')
        self.temperature, self._inv_tau = (None if inv is None else tau), inv

    def set_ensemble(self, pass_s, pass_e):
        """the span posterior as a Bayesian model average: pass_s / pass_e f32 [K, N, ld] on the updater's device, 1 <= K <= 16, the
        logits of K stochastic passes (a McBank's planes).  While set, query(), span_marginals() and mbr_label() read the mixture of
        the passes' posteriors, each weighted by its evidence of the answers (hual_al_ensemble_query / hual_al_ensemble_label) -
        under noise=eps behind one hual_al_noisy_tilt per plane -, set_temperature scales the planes as it scales the deterministic
        logits, and label_gain(), session(), calibrate() and evidence_grid() raise: they have no ensemble form.  None (both): off
        again - every launch and bit as it was.  score() and renew() never read it; tilt() keeps tilting the deterministic logits.
        Either way the call forgets the scaled rows and the tilt the updater holds (tilt_eps is None after it), and while an
        ensemble is set a tilt() between two of its noisy readers makes the second tilt the passes again: the chain has one slot
        per stage."""
        if (pass_s is None) != (pass_e is None):
            raise ValueError('set_ensemble: pass_s and pass_e are both tensors or both None')
        if pass_s is not None:
            ok = (torch.is_tensor(pass_s) and torch.is_tensor(pass_e) and pass_s.dtype == torch.float32 and pass_e.dtype == torch.float32
                  and pass_s.dim() == 3 and pass_e.shape == pass_s.shape and tuple(pass_s.shape[1:]) == (self.N, self.ld)
                  and 1 <= pass_s.shape[0] <= lib.AL_ENS_MAX_K and pass_s.is_contiguous() and pass_e.is_contiguous()
                  and pass_s.device == self.dev and pass_e.device == self.dev)
            if not ok:
                raise lib.HualError('set_ensemble: pass_s / pass_e must be contiguous float32 [K, N, ld] = [1..%d, %d, %d] on the updater\'s device'
                                    % (lib.AL_ENS_MAX_K, self.N, self.ld))
        self._drop('source')
        if pass_s is not None:
            self._chain['source'] = (pass_s, pass_e)

    def _no_ensemble(self, what):
        if self._posterior_source() is not self._det:
            raise lib.HualError('%s has no ensemble form: call set_ensemble(None, None) first' % what)

    def _free_set(self):
        """a hual_al_set over the same vlen / tlen WITHOUT answers: what the family's launches take beside tilted rows"""
        if getattr(self, '_free', None) is None:                 # (made once: vlen and tlen are the updater's for good)
            self._free = (torch.zeros(self.N + 1, dtype=torch.int32, device=self.dev), torch.zeros(1, dtype=torch.int32, device=self.dev),
                          torch.zeros(1, dtype=torch.int8, device=self.dev))
            p = lib.ptr
            self.free_set = lib.hual_al_set(self.N, self.ld, p(self.vlen).value, p(self.tlen).value, *[p(x).value for x in self._free])
        return self.free_set

    def _scaled(self, src):
        """(s, e) of `src` as the launches read them: the very same tensors, or under a temperature their float32 products with 1 / tau"""
        made = self._chain.get('scaled')
        if made is None or made[0] is not src:
            s, e = src
            if self._inv_tau is not None:
                k = float(self._inv_tau)                         # (a python scalar: torch multiplies in float32, by float32(1 / tau))
                s, e = (s * k).contiguous(), (e * k).contiguous()
            made = self._chain['scaled'] = (src, s, e)
        return made[1:]

    def _tilted(self, src, eps, fresh=False):
        """(s_t, e_t, log_evidence) of the scaled `src` tilted by the set's answers under eps, shaped as `src` is ([N, ld] and [N], or
        [K, N, ld] and [K, N]): hual_al_noisy_tilt, one launch per plane - launched only where the chain holds none from these rows at
        this eps, or with fresh"""
        s, e = self._scaled(src)
        made = self._chain.get('tilted')
        if fresh or made is None or made[0] is not s or made[1] != eps:
            if s.dim() == 2:
                st, et, lev = lib.al_noisy_tilt(self.set, s, e, self.tlen_h, eps)
            else:                                                # (the same launch per plane, into one tensor per output)
                st, et, lev = torch.zeros_like(s), torch.zeros_like(e), torch.empty(s.shape[:-1], device=self.dev)
                for k in range(s.shape[0]):
                    lib.al_noisy_tilt(self.set, s[k], e[k], self.tlen_h, eps, out=(st[k], et[k], lev[k]))
            made = self._chain['tilted'] = (s, eps, st, et, lev)
            self._last_eps = eps
            if src is self._det:
                self.s_t, self.e_t, self.log_evidence, self.tilt_eps = st, et, lev, eps
        return made[2:]

    def _logits(self):
        """(s, e) the deterministic posterior's launches read: the deterministic logits, or under a temperature their float32 products
        with 1 / tau"""
        return self._scaled(self._det)

    def _reads(self, noise):
        """(set, s, e, logw) a launch of the span posterior takes: the updater's set, the scaled source and no prior weight; or under
        noise = eps the set without answers, the source tilted by eps (tilted here unless it already is) and its log_evidence - for
        an ensemble [K, N], the logarithms of the passes' weights: pass k's evidence of the noisy answers is exactly its weight"""
        if noise is None:
            return (self.set,) + self._scaled(self._posterior_source()) + (None,)
        return (self._free_set(),) + self._tilted(self._posterior_source(), check_noise(noise))

    def _launch(self, what, noise, **kw):
        """one launch of the span posterior on what _reads(noise) gives - `what` = 'query', 'marginals' or 'label': lib's wrapper on the
        deterministic rows, or its ensemble twin on the passes' planes and weights -> (the plain wrapper's tuple, whichever ran - the
        ensemble has no agree -; what only the ensemble query leaves: (weight, log_evidence, expected_entropy, span_bald, status), else
        None)"""
        aset, s, e, logw = self._reads(noise)
        if self._posterior_source() is self._det:
            plain = lib.al_query if what == 'query' else lib.al_span_marginals if what == 'marginals' else lib.al_mbr_label
            return plain(aset, s, e, self.tlen_h, **kw), None
        if what == 'label':
            return lib.al_ensemble_label(aset, s, e, self.tlen_h, logw=logw, **kw), None
        o = lib.al_ensemble_query(aset, s, e, self.tlen_h, logw=logw, frames=kw.get('frames', False), marginals=what == 'marginals')
        if what == 'marginals':
            return (o[6], o[7], o[11]), None
        return (o[2], o[3], o[4], o[5], o[8], None), (o[0], o[1], o[9], o[10], o[11])

    def evidence_grid(self, taus, eps, sel=None):
        """ln P(the set's answers | softmax(s0 / tau), softmax(e0 / tau), eps) per sample on the grid taus x eps and its sum over the
        set (hual_al_evidence_grid, lib.al_evidence_grid) on the updater's set and UNSCALED deterministic logits, whatever
        set_temperature holds.  taus: 1 to 32 temperatures > 0, handed on as float32(1 / tau); eps: 1 to 16 error rates in (0, 0.5];
        sel: None or the sample ids (numpy).  Leaves and returns (ev_table f64 [N, A * B], ev_status i32 [N], ev_total f64 [A * B],
        ev_counts i32 [4]) as device tensors."""
        self._no_ensemble('evidence_grid()')
        inv = np.array([np.float32(1.0 / float(t)) for t in np.asarray(taus, dtype=np.float64).reshape(-1)], dtype=np.float32)
        sel_d = None if sel is None else torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int32)).to(self.dev)
        self.ev_table, self.ev_status, self.ev_total, self.ev_counts = lib.al_evidence_grid(
            self.set, self._s0, self._e0, self.tlen_h, inv, np.asarray(eps, dtype=np.float32).reshape(-1), sel=sel_d)
        return self.ev_table, self.ev_status, self.ev_total, self.ev_counts

    def calibrate(self, taus=None, eps=None, refine=2, sel=None, min_answers=32, at_eps=None):
        """fit the temperature and the annotator's error rate to the set's answers by their evidence: the pair that maximises
        L(tau, eps) = the sum over the samples of ln P(the answers | softmax(s0 / tau), softmax(e0 / tau), eps) on a grid, then on
        `refine` finer grids around the best cell - one evidence_grid() launch each.
        taus / eps: the coarse grid (None: CALIB_TAUS, 2^(k/4) for k = -8..8, and CALIB_EPS); an axis of one value stays fixed.  Every
        zoom grid is geometric in tau and in the odds eps / (1 - eps), spans the best cell's neighbours on both axes (one step past
        the edge where the best cell lies on it), is clamped to tau > 0 and eps in [CALIB_MIN_EPS, 0.5], and holds the best cell
        itself: the best total never decreases from grid to grid.  sel: None or the sample ids (numpy) to fit on.
        at_eps: the error rate of the uncalibrated posterior the fit is compared with (None: the eps of the tilt the updater holds or
        last held); the cell (tau = 1, at_eps) is part of the coarse grid.
        -> None with fewer than min_answers answers inside their clips (on the host, before any launch; and again among the rows the
        launch summed): nothing is extrapolated from three clicks.  Else a dict: tau, eps (python floats; eps a float32 widened, as
        check_noise returns it), log_evidence (the best total of the last grid), per_answer = exp(log_evidence / answers), the
        geometric-mean likelihood of an answer, at_default = the total at (1, at_eps) (None without an at_eps), rows, answers,
        excluded (of the last grid: a row poisoned at one of a grid's temperatures is left out of that whole grid), and grids = every
        launched (taus, eps, totals [A, B]) as numpy arrays."""
        self._no_ensemble('calibrate()')
        rows = np.arange(self.N) if sel is None else np.asarray(sel, dtype=np.int64)
        if rows.ndim != 1 or rows.size < 1 or rows.min() < 0 or rows.max() >= self.N:
            raise ValueError('calibrate: sel holds sample ids in [0, N)')
        refine = int(refine)
        if refine < 0:
            raise ValueError('calibrate: refine >= 0')
        if at_eps is None:
            at_eps = self.tilt_eps if self.tilt_eps is not None else self._last_eps
        at_eps = None if at_eps is None else check_noise(at_eps)
        tg = np.unique(np.asarray(CALIB_TAUS if taus is None else taus, dtype=np.float64).reshape(-1))
        eg = np.unique(np.array([check_noise(e) for e in np.asarray(CALIB_EPS if eps is None else eps).reshape(-1)], dtype=np.float64))
        if tg.size < 1 or not (np.isfinite(tg).all() and (tg > 0).all()):
            raise ValueError('calibrate: the temperatures must be finite and > 0')
        fixed_tau, fixed_eps = tg.size == 1, eg.size == 1
        nt, ne = min(max(tg.size, 3), lib.AL_GRID_MAX_TAU - 1), min(max(eg.size, 3), lib.AL_GRID_MAX_EPS - 1)
        own_t, own_e = tg, eg                                    # the cells the fit may choose: the caller's
        if at_eps is not None:                                   # the uncalibrated cell rides in the coarse grid
            tg, eg = np.unique(np.append(tg, 1.0)), np.unique(np.append(eg, at_eps))
        if tg.size > lib.AL_GRID_MAX_TAU or eg.size > lib.AL_GRID_MAX_EPS:
            raise ValueError('calibrate: at most %d temperatures and %d error rates per grid (the uncalibrated cell included)'
                             % (lib.AL_GRID_MAX_TAU, lib.AL_GRID_MAX_EPS))
        inside = sum(1 for i in rows for f, _ in self.aps[i] if 0 <= f < min(int(self.vlen_h[i]), int(self.tlen_h[i])))
        if inside < int(min_answers):
            return None
        grids, at_default = [], None
        for level in range(refine + 1):
            _, _, total, counts = self.evidence_grid(tg, eg, sel=None if sel is None else rows)
            tot, cnt = total.cpu().numpy().reshape(tg.size, eg.size), counts.cpu().numpy()
            grids.append((tg.copy(), eg.copy(), tot))
            if cnt[0] < 1 or cnt[1] < int(min_answers):
                return None
            # the first cell of maximal total, the launch's own rule (counts[3]) - among the caller's cells where the uncalibrated
            # cell brought a row or a column of its own into the coarse grid
            own = np.isin(tg, own_t)[:, None] & np.isin(eg, own_e)[None, :] if level == 0 else np.ones(tot.shape, dtype=bool)
            ia, ib = divmod(int(np.argmax(np.where(own, tot, -np.inf))), eg.size)
            if level == 0 and at_eps is not None:
                at_default = float(tot[int(np.searchsorted(tg, 1.0)), int(np.searchsorted(eg, at_eps))])
            if level == refine:
                break
            if fixed_tau:
                tg = tg[ia:ia + 1]
            else:
                tg = np.unique(np.append(_zoom_axis(tg, ia, nt, 0.0, float('inf')), tg[ia]))
            if fixed_eps:
                eg = eg[ib:ib + 1]
            else:
                odds = _zoom_axis(eg / (1.0 - eg), ib, ne, CALIB_MIN_EPS / (1.0 - CALIB_MIN_EPS), 1.0)
                eg = np.unique(np.array([check_noise(min(o / (1.0 + o), 0.5)) for o in odds] + [eg[ib]], dtype=np.float64))
        best = float(tot[ia, ib])
        return dict(tau=float(tg[ia]), eps=float(eg[ib]), log_evidence=best, per_answer=float(np.exp(best / int(cnt[1]))),
                    at_default=at_default, rows=int(cnt[0]), answers=int(cnt[1]), excluded=int(cnt[2]), grids=grids)

    def tilt(self, eps):
        """the set's answers folded into the deterministic logits under an annotator who errs with probability eps in (0, 0.5]
        (hual_al_noisy_tilt, one launch over the whole set).  Leaves s_t, e_t (f32 [N, ld], the tilted rows), log_evidence (f32 [N]:
        ln P(the answers | the model, eps), NaN on a poisoned row), free_set (a hual_al_set over the same vlen / tlen WITHOUT answers:
        what the family's launches take beside the tilted rows) and tilt_eps; set_active_points invalidates them."""
        self._tilted(self._det, check_noise(eps), fresh=True)
        self._free_set()

    def score(self, coff_uncert):
        lib.al_score(self.set, self._s0, self._e0, coff_uncert, (self.sprob, self.eprob, self.uncert_frame, self.uncert_video, self.observe),
                     pair=self.logits[2:] if self.logits is not None else None, bank=self.bank_c,
                     info=self.bank.info_c if self.bank is not None else None, K=self.K, stat=self.stat)

    def query(self, frames=True, noise=None):
        """the span posterior given the set's answered active points and the frame of most expected information gain (hual_al_query,
        one launch) on the updater's set and deterministic logits - of the records or of the bank.  Leaves incl, gain (f32 [N, ld];
        None with frames=False), query_point (i32 [N]), query_gain, post_entropy and agree (f32 [N]) as device tensors.
        noise=eps: the posterior under an annotator who errs with probability eps - the same launch on the tilted rows (tilt()) and
        the set without answers.  gain / query_gain are then the information a NOISY answer carries, h2(eps + (1 - 2 eps) q) - h2(eps)
        bits, from incl in float64, stored as float32 (frames=True is needed); query_point stays the kernel's - the same maximiser,
        q nearest 1/2 -; agree is None: log_evidence (tilt()) is the quantity to read.
        With an ensemble set (set_ensemble) the same fields are read from the model average over the passes (hual_al_ensemble_query,
        one launch; under noise behind one tilt per plane): post_entropy is the mixture's, agree is None, and the call also leaves and
        returns - as a dict - weight (f32 [N, K]), log_evidence (f32 [N], ln P(the answers | the ensemble); the attribute is
        ens_log_evidence), expected_entropy and span_bald (f32 [N], bits).  Without one it returns None."""
        if noise is not None and not frames:
            raise ValueError('query(noise=) computes the gain of a noisy answer from incl: it needs frames=True')
        (self.incl, self.gain, self.query_point, self.query_gain, self.post_entropy, self.agree), ens = self._launch('query', noise, frames=frames)
        if ens is not None:
            self.weight, self.ens_log_evidence, self.expected_entropy, self.span_bald, self.ens_status = ens
            ens = dict(weight=self.weight, log_evidence=self.ens_log_evidence, expected_entropy=self.expected_entropy,
                       span_bald=self.span_bald)
        if noise is not None:
            eps = check_noise(noise)

            def h2(x):
                x = x.clamp(1e-300, 1.0)
                y = (1.0 - x).clamp(1e-300, 1.0)
                return -(x * torch.log2(x) + y * torch.log2(y))
            ch = (h2(eps + (1.0 - 2.0 * eps) * self.incl.double()) - h2(torch.tensor(eps, dtype=torch.float64, device=self.dev))).clamp_min(0.0)
            live = self.query_point >= 0
            at = ch.gather(1, self.query_point.clamp_min(0).long()[:, None])[:, 0]
            self.gain = torch.where(live[:, None], ch, torch.zeros_like(ch)).float()
            self.query_gain = torch.where(live, at, torch.full_like(at, -1.0)).float()
            self.agree = None
        return ens

    def session(self, gt_idx, max_questions, stop_entropy=None, min_gain=0.0, noise=None, flips=None, budget=None, sel=None):
        """an annotation session per sample (hual_al_session, one launch): up to max_questions (1..16) questions, each the frame of
        most expected information gain under the span posterior given every answer so far - query()'s frame on the grown list -,
        answered from the ground-truth spans gt_idx (int [N, 2], frame indices, inclusive), until the posterior's entropy is at most
        stop_entropy bits (None: never), the best gain is at most min_gain bits (0: only a collapsed posterior stops), the budget is
        spent, or the row is contradictory or poisoned.  noise=eps: the posterior under an annotator who errs with probability eps
        (tilt() + query() per step, in the kernel); flips: None or uint [N], bit k flips the k-th answer of the sample's session - the
        simulated annotator's errors; budget: None or int [N], per-sample caps (clamped to [0, max_questions]); sel: None (every
        sample) or the sample ids (numpy) to run.
        Leaves asked (i32 [N, Q]), answers (i8 [N, Q]), q_asked, session_gain (f32 [N, Q]), entropy_path (f32 [N, Q + 1]), n_asked and
        stop_reason (i32 [N]; lib.AL_STOP_REASONS) as device tensors - rows outside sel and unused slots hold -1 - and installs the
        extended lists with set_active_points (which invalidates a tilt).  A sample whose answered points plus budget exceed
        lib.AL_SESSION_MAX_POINTS is refused here, on the host, where the lists are known.
        Returns numpy (asked, answers, n_asked)."""
        self._no_ensemble('session()')
        Q = int(max_questions)
        if not 1 <= Q <= lib.AL_SESSION_MAX_Q:
            raise ValueError('session: max_questions must lie in [1, %d]' % lib.AL_SESSION_MAX_Q)
        if not float(min_gain) >= 0.0:
            raise ValueError('session: min_gain >= 0')
        eps = 0.0 if noise is None else check_noise(noise)
        gt = np.ascontiguousarray(gt_idx, dtype=np.int32)
        if gt.shape != (self.N, 2):
            raise ValueError('session: gt_idx must hold N = %d spans' % self.N)
        rows = np.arange(self.N) if sel is None else np.asarray(sel, dtype=np.int64)
        if rows.ndim != 1 or rows.size < 1 or rows.min() < 0 or rows.max() >= self.N:
            raise ValueError('session: sel holds sample ids in [0, N)')
        cap = np.full(self.N, Q, dtype=np.int64) if budget is None else np.clip(np.asarray(budget, dtype=np.int64), 0, Q)
        if cap.shape != (self.N,):
            raise ValueError('session: budget must hold N = %d caps' % self.N)
        for i in rows:
            if len(self.aps[i]) + int(cap[i]) > lib.AL_SESSION_MAX_POINTS:
                raise ValueError('session: sample %d holds %d answered points: with a budget of %d that exceeds the %d a session keeps'
                                 % (i, len(self.aps[i]), int(cap[i]), lib.AL_SESSION_MAX_POINTS))

        def dev32(x):
            return torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)
        flip_d = None if flips is None else dev32(np.asarray(flips, dtype=np.uint32).view(np.int32))
        (self.asked, self.answers, self.q_asked, self.session_gain, self.entropy_path, self.n_asked,
         self.stop_reason) = lib.al_session(self.set, *self._logits(), self.tlen_h, dev32(gt), Q,
                                            sel=None if sel is None else dev32(rows.astype(np.int32)),
                                            budget=None if budget is None else dev32(cap.astype(np.int32)),
                                            stop_entropy=-1.0 if stop_entropy is None else float(stop_entropy), min_gain=float(min_gain),
                                            eps=eps, flip=flip_d)
        asked, answers, n_asked = self.asked.cpu().numpy(), self.answers.cpu().numpy(), self.n_asked.cpu().numpy()
        aps = list(self.aps)                                     # (a new outer list and new rows: the caller's lists are not touched)
        for i in set(int(i) for i in rows):
            aps[i] = list(aps[i]) + [(int(asked[i, k]), bool(answers[i, k])) for k in range(int(n_asked[i]))]
        self.set_active_points(aps)
        return asked, answers, n_asked

    def session_label(self, gt_idx, max_questions, thresholds=(0.3, 0.5, 0.7), stop_hit=None, stop_at=0.7, stop_entropy=None, min_gain=0.0,
                      noise=None, flips=None, budget=None, sel=None):
        """session() that knows what the annotation is for (hual_al_session_label, one launch): after every pass the session also
        takes the minimum-Bayes-risk label of the list so far (mbr_label()'s) and that label's hit probability at the IoU thresholds
        `thresholds` (lib.hit_thresholds, at most 4; hit_label()'s cand_hit of that one span), and with stop_hit=p in (0, 1] it stops
        as 'reliable' - before the entropy, gain and budget rules - once the stored float32 probability at the threshold stop_at (one
        of `thresholds`) is at least p.  stop_hit=None: the rule is off and the session is session()'s bit for bit.  Every other
        argument, the refusals and the returned numpy (asked, answers, n_asked) are session()'s.
        Leaves session()'s tensors and label_path (i32 [N, Q + 1, 2]), label_conf_path (f32 [N, Q + 1]) and label_hit_path (f32
        [N, Q + 1, M]) as device tensors: slot k is the pass before question k, slot n_asked the final label - what mbr_label() gives
        on the installed lists -; unused slots, passes that were not live and rows outside sel hold -1.  Installs the extended lists
        with set_active_points.  It has no ensemble form."""
        self._no_ensemble('session_label()')
        Q = int(max_questions)
        if not 1 <= Q <= lib.AL_SESSION_MAX_Q:
            raise ValueError('session_label: max_questions must lie in [1, %d]' % lib.AL_SESSION_MAX_Q)
        if not float(min_gain) >= 0.0:
            raise ValueError('session_label: min_gain >= 0')
        thr = lib.hit_thresholds(thresholds)
        at = lib.hit_thresholds((stop_at,))[0]
        if at not in thr:
            raise ValueError('session_label: stop_at must be one of the thresholds')
        if stop_hit is not None and not 0.0 < float(stop_hit) <= 1.0:
            raise ValueError('session_label: stop_hit is None or a probability in (0, 1]')
        eps = 0.0 if noise is None else check_noise(noise)
        gt = np.ascontiguousarray(gt_idx, dtype=np.int32)
        if gt.shape != (self.N, 2):
            raise ValueError('session_label: gt_idx must hold N = %d spans' % self.N)
        rows = np.arange(self.N) if sel is None else np.asarray(sel, dtype=np.int64)
        if rows.ndim != 1 or rows.size < 1 or rows.min() < 0 or rows.max() >= self.N:
            raise ValueError('session_label: sel holds sample ids in [0, N)')
        cap = np.full(self.N, Q, dtype=np.int64) if budget is None else np.clip(np.asarray(budget, dtype=np.int64), 0, Q)
        if cap.shape != (self.N,):
            raise ValueError('session_label: budget must hold N = %d caps' % self.N)
        for i in rows:
            if len(self.aps[i]) + int(cap[i]) > lib.AL_SESSION_MAX_POINTS:
                raise ValueError('session_label: sample %d holds %d answered points: with a budget of %d that exceeds the %d a session keeps'
                                 % (i, len(self.aps[i]), int(cap[i]), lib.AL_SESSION_MAX_POINTS))

        def dev32(x):
            return torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)
        flip_d = None if flips is None else dev32(np.asarray(flips, dtype=np.uint32).view(np.int32))
        (self.asked, self.answers, self.q_asked, self.session_gain, self.entropy_path, self.n_asked, self.stop_reason, self.label_path,
         self.label_conf_path, self.label_hit_path) = lib.al_session_label(
            self.set, *self._logits(), self.tlen_h, dev32(gt), Q, thresholds=thresholds, stop_m=thr.index(at),
            stop_hit=-1.0 if stop_hit is None else float(stop_hit), sel=None if sel is None else dev32(rows.astype(np.int32)),
            budget=None if budget is None else dev32(cap.astype(np.int32)),
            stop_entropy=-1.0 if stop_entropy is None else float(stop_entropy), min_gain=float(min_gain), eps=eps, flip=flip_d)
        asked, answers, n_asked = self.asked.cpu().numpy(), self.answers.cpu().numpy(), self.n_asked.cpu().numpy()
        aps = list(self.aps)                                     # (a new outer list and new rows: the caller's lists are not touched)
        for i in set(int(i) for i in rows):
            aps[i] = list(aps[i]) + [(int(asked[i, k]), bool(answers[i, k])) for k in range(int(n_asked[i]))]
        self.set_active_points(aps)
        return asked, answers, n_asked

    def design(self, max_points, min_gain=0.0, stop_entropy=None, noise=None, forced=None, sel=None):
        """the frames to ask TOGETHER about every sample (hual_al_design, one launch): for an annotator who is not in the loop - a
        labelling tool, a crowd batch, one viewing of the clip - a greedy design of up to max_points (1..16) frames under the span
        posterior given the set's answered active points.  The answers are a function of the span, so the information a set of frames
        D carries is the entropy of its answer vector, I(D); step m takes the first frame of maximal I(D + t) - step 0 is query()'s
        frame and gain - until the best marginal gain is at most min_gain bits (0: only a design that has nothing left to learn stops),
        the expected entropy left, post_entropy - I(D), is at most stop_entropy bits (None: never), max_points frames are placed, or
        the row is contradictory or poisoned.  forced: None or int [N, k], k <= max_points - a row's leading entries >= 0 are the first
        frames of its design, placed without a stop test (-1 ends them; a frame beyond the clip is ignored; a repeated or already
        answered one stays with 0 bits): how a hand-made grid or a bisection schedule is scored.  sel: None (every sample) or the
        sample ids (numpy) to run.
        noise=eps: the posterior under an annotator who errs with probability eps - the same launch on the tilted rows (tilt()) and the
        set without answers, as query().  design_info is then the information of EXACT answers to the new questions: an upper bound on
        what noisy answers to them carry.
        Leaves design_frames (i32 [N, M], in the order chosen), design_info (f32 [N, M]: the information of the first m + 1 frames,
        bits), design_entropy (f32 [N]: query()'s post_entropy), n_design and design_stop (i32 [N]; lib.AL_STOP_REASONS) as device
        tensors - rows outside sel and unused slots hold -1.  Installs nothing: no answer exists yet.
        Returns numpy (frames, n_design)."""
        self._no_ensemble('design()')
        M = int(max_points)
        if not 1 <= M <= lib.AL_DESIGN_MAX_M:
            raise ValueError('design: max_points must lie in [1, %d]' % lib.AL_DESIGN_MAX_M)
        if not float(min_gain) >= 0.0:
            raise ValueError('design: min_gain >= 0')
        if stop_entropy is not None and not float(stop_entropy) >= 0.0:
            raise ValueError('design: stop_entropy is None or bits >= 0')
        rows = np.arange(self.N) if sel is None else np.asarray(sel, dtype=np.int64)
        if rows.ndim != 1 or rows.size < 1 or rows.min() < 0 or rows.max() >= self.N:
            raise ValueError('design: sel holds sample ids in [0, N)')
        forced_h = None
        if forced is not None:
            f = np.asarray(forced, dtype=np.int64)
            if f.ndim != 2 or f.shape[0] != self.N or not 1 <= f.shape[1] <= M:
                raise ValueError('design: forced must hold N = %d rows of at most max_points frames' % self.N)
            forced_h = np.full((self.N, M), -1, dtype=np.int32)
            forced_h[:, :f.shape[1]] = np.clip(f, -1, 2 ** 31 - 1)

        def dev32(x):
            return torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)
        aset, s, e, _ = self._reads(noise)
        (self.design_frames, self.design_info, self.design_entropy, self.n_design,
         self.design_stop) = lib.al_design(aset, s, e, self.tlen_h, M, sel=None if sel is None else dev32(rows.astype(np.int32)),
                                           forced=None if forced_h is None else dev32(forced_h), min_gain=float(min_gain),
                                           stop_entropy=-1.0 if stop_entropy is None else float(stop_entropy))
        return self.design_frames.cpu().numpy(), self.n_design.cpu().numpy()

    def label_gain(self, frames=True, cand=None, noise=None):
        """per frame, the tIoU the minimum-Bayes-risk label is expected to gain from the frame's answer under the span posterior given
        the set's answered active points (hual_al_label_gain, one launch over the whole set) on the updater's set and deterministic
        logits - of the records or of the bank, as query().  cand: device i32 [N, M], the only frames to evaluate (None: every frame).
        Leaves gain (f32 [N, ld]; None with frames=False; in place of the row of bits query() leaves under that name), ask_point
        (i32 [N]), ask_gain and label_value (f32 [N]) as device tensors.
        noise=eps: the gain from a NOISY answer (hual_al_label_gain_noisy, one launch) on the rows tilted by eps (tilt())."""
        self._no_ensemble('label_gain()')
        aset, s, e, _ = self._reads(noise)
        if noise is None:
            out = lib.al_label_gain(aset, s, e, self.tlen_h, cand=cand, frames=frames)
        else:
            out = lib.al_label_gain_noisy(aset, s, e, self.tlen_h, check_noise(noise), cand=cand, frames=frames)
        self.gain, self.ask_point, self.ask_gain, self.label_value = out

    def span_marginals(self, noise=None):
        """the start and end marginals of the span posterior given the set's answered active points (hual_al_span_marginals, one launch
        over the whole set) on the updater's set and deterministic logits - of the records or of the bank, as query().  Leaves y_start,
        y_end (f32 [N, ld]) and marg_status (i32 [N]; 1 = live) as device tensors.
        noise=eps: the marginals of the posterior under an annotator who errs with probability eps - the same launch on the rows
        tilted by eps (tilt()) and the set without answers.
        With an ensemble set: the marginals of the model average, sum_k w_k of the passes' (hual_al_ensemble_query, one launch)."""
        (self.y_start, self.y_end, self.marg_status), _ = self._launch('marginals', noise)

    def mbr_label(self, sel, old_idx, noise=None):
        """the minimum-Bayes-risk pseudo-label of the samples `sel` (sample ids, numpy) under the span posterior given the set's
        answered active points (hual_al_mbr_label, one launch) on the updater's set and deterministic logits - of the records or of the
        bank, as query().  old_idx: int [N, 2].  Returns numpy (new_idx i32 [N, 2], conf f32 [N], old_conf f32 [N]): the label, its
        expected tIoU and the old span's; rows outside `sel`, and rows that give no label, hold -1.
        noise=eps: the label under an annotator who errs with probability eps - the same launch on the rows tilted by eps (tilt())
        and the set without answers: any span of the clip, and only a poisoned row gives none.
        With an ensemble set: the label of maximal expected tIoU under the model average (hual_al_ensemble_label, one launch)."""
        sel_d = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int32)).to(self.dev)
        old_d = torch.from_numpy(np.ascontiguousarray(old_idx, dtype=np.int32)).to(self.dev)
        (new_d, conf, old_conf), _ = self._launch('label', noise, sel=sel_d, old_idx=old_d)
        return new_d.cpu().numpy(), conf.cpu().numpy(), old_conf.cpu().numpy()

    def hit_label(self, sel=None, cand=None, thresholds=(0.3, 0.5, 0.7), best=True, noise=None):
        """label reliability: P(IoU(span, truth) >= m | the answers) of the spans `cand` (int [N, k, 2], numpy or a device tensor, k <=
        16; None: none) of the samples `sel` (sample ids, numpy; None: all) under the span posterior given the set's answered active
        points, at the IoU thresholds `thresholds` (lib.hit_thresholds), and with best=True per threshold the member of the consistent
        set that maximises it (hual_al_hit_label, one launch) on the updater's set and deterministic logits - of the records or of the
        bank, as query().  Leaves cand_hit (f32 [N, k, M]; None without cand), hit_best_idx (i32 [N, M, 2]) and hit_best_prob (f32
        [N, M]; both None with best=False: the launch then does not search) as device tensors; rows outside `sel`, slots that are no
        span of the clip and rows that give no probability hold -1.
        noise=eps: the same launch on the rows tilted by eps (tilt()) and the set without answers - every span of the clip is then
        consistent, and only a poisoned row gives none.  It has no ensemble form."""
        self._no_ensemble('hit_label()')
        aset, s, e, _ = self._reads(noise)
        sel_d = None if sel is None else torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int32)).to(self.dev)
        if cand is not None and not torch.is_tensor(cand):
            cand = torch.from_numpy(np.ascontiguousarray(cand, dtype=np.int32)).to(self.dev)
        self.cand_hit, found = lib.al_hit_label(aset, s, e, self.tlen_h, thresholds=thresholds, sel=sel_d, cand=cand, best=best)
        self.hit_best_idx, self.hit_best_prob = found if found is not None else (None, None)

    def renew(self, sel, old_idx, coff):
        """sel: sample ids (numpy); old_idx: int [N,2]; returns new_idx int32 [N,2] (valid for the selected rows)"""
        sel_d = torch.from_numpy(np.ascontiguousarray(sel, dtype=np.int32)).to(self.dev)
        old_d = torch.from_numpy(np.ascontiguousarray(old_idx, dtype=np.int32)).to(self.dev)
        new_d = torch.full((self.N, 2), -1, device=self.dev, dtype=torch.int32)
        c6 = (ctypes.c_double * 6)(*[float(x) for x in coff[:6]])
        lib.check(self._lib.hual_al_renew(ctypes.byref(self.set), lib.ptr(sel_d), int(len(sel)), lib.ptr(self.sprob),
                                          lib.ptr(self.eprob), lib.ptr(old_d), c6, lib.ptr(new_d), lib.stream_ptr()))
        return new_d.cpu().numpy()


POSTERIOR = ('deterministic', 'ensemble')
RANK_BY = ('uncert_video', 'span_risk')
RANK_BY_ENSEMBLE = ('span_bald',)      # with posterior='ensemble' only (check_round)
RANK_BY_HIT = ('label_miss',)          # label reliability (LabelUpdater.hit_label): the deterministic posterior only
RANK_BY_GRAD = ('egl',)                # the expected gradient length of the records (infer_trainset(grad_bank=)), largest first
OBSERVE_BY = ('uncert_frame', 'info_gain')
RENEW_BY = ('heuristic', 'posterior')
RENEW_BY_HIT = ('hit_prob',)           # the same
ACQUIRE_BY = (None, 'label_gain')
CALIBRATE = (None, 'evidence')
HIT_IOUS = (0.3, 0.5, 0.7)             # the thresholds of the round's hit_label launches, in column order; hit_iou is one of them
HIT_MARGIN = 1e-6                      # renew_by='hit_prob' moves a label only for more than this: below it two probabilities are a tie

# check_round's result: the switches of a round as update_labels works from them - the enumerations as given; Q, the questions per
# clip, an int; stop_entropy, noise and temperature floats or None; flip None or (rate, Generator); reads_posterior: one of the span
# posterior's readers is on; questions_at_once: M, the frames a selected sample is asked together; hit_iou: the threshold of HIT_IOUS
# that rank_by='label_miss', renew_by='hit_prob' and stop_hit decide at
_RoundFields = collections.namedtuple('RoundPolicy', 'posterior rank_by observe_by renew_by acquire_by Q stop_entropy noise temperature '
                                                     'calibrate flip reads_posterior questions_at_once hit_iou')


class RoundPolicy(_RoundFields):
    """the tuple of a round's switches, and beside it - attributes, not fields: the tuple of a round without them is the tuple it
    was - stop_hit: None, or the hit probability of the label at hit_iou at which a session stops; select_by / descriptors /
    diversity_init: how the asked half is chosen from the ranking (None: its top half; 'kcenter': diverse_select on the descriptors;
    'badge': badge_select on them - D^2 sampling from the origin under selection_seed; with diversity_init='answered' around the
    clips that already hold an active point)"""
    stop_hit = None
    select_by = None
    descriptors = None
    diversity_init = None
    selection_seed = None

    def __new__(cls, *fields, stop_hit=None, select_by=None, descriptors=None, diversity_init=None, selection_seed=None):
        pol = super().__new__(cls, *fields)
        pol.stop_hit = stop_hit
        pol.select_by, pol.descriptors, pol.diversity_init = select_by, descriptors, diversity_init
        pol.selection_seed = selection_seed
        return pol


SELECT_BY = (None, 'kcenter', 'badge')
DIVERSITY_INIT = (None, 'answered')


def rank_weights(order):
    """the selection weights of a ranking: w[i] = float32((N - rank_i) / N), computed in float64, rank_i the position of i in
    `order` - 1 for the first-ranked clip, 1 / N for the last.  Ranks, not scores: scale-free, and valid for every rank_by whichever
    way its scalar points."""
    order = np.asarray(order)
    N = len(order)
    if sorted(order.tolist()) != list(range(N)):
        raise ValueError('order must be a permutation of range(N)')
    rank = np.empty(N, dtype=np.int64)
    rank[order] = np.arange(N)
    return ((N - rank).astype(np.float64) / N).astype(np.float32)


def _diverse(desc, order, n_select, weighted=True, init=None):
    """diverse_select's launch -> (picks without the -1 of an exhausted selection, picked, pick_dist, mind: the launch's tensors)"""
    if not (torch.is_tensor(desc) and desc.dim() == 2 and desc.dtype == torch.float32):
        raise ValueError('descriptors: a float32 [N, D] device tensor')
    order = np.asarray(order)
    N = int(desc.shape[0])
    if len(order) != N:
        raise ValueError('descriptors: %d rows for %d ranked samples' % (N, len(order)))
    init = None if init is None or len(init) == 0 else np.asarray(init, dtype=np.int64)
    if weighted:
        w = rank_weights(order)
    elif init is None:                                           # plain k-center started at order[0]: the one larger weight wins step 0
        rank_weights(order)                                      # (the permutation check)
        w = np.full(N, 0.5, dtype=np.float32)                    # (equal weights: every later step is plain k-center - 0.5 x is exact)
        w[order[0]] = 1.0
    else:                                                        # plain k-center around the given centers: no weights at all
        rank_weights(order)
        w = None
    w_d = None if w is None else torch.from_numpy(w).to(desc.device)
    picked, dist, mind, _ = lib.kcenter_select(desc, n_select, weight=w_d, init=init)
    picks = picked.cpu().numpy().astype(np.int64)
    return picks[picks >= 0], picked, dist, mind


def diverse_select(desc, order, n_select, weighted=True, init=None):
    """core-set selection of the clips to ask: n_select greedy k-center picks in the descriptor space (lib.kcenter_select, one call),
    weighted by the ranking.  desc: device f32 [N, D] (DeviceDataset.clip_descriptors()); order: the ranking of the N samples, best
    first (update_labels' order, whatever rank_by made it).  weighted: the weights are rank_weights(order), so step s asks the clip
    of maximal weight x squared distance to the clips asked so far, and among exact ties - duplicate descriptors - the better-ranked
    one; the first pick is order[0].  weighted=False: plain k-center started at order[0] - weight 1 for order[0] and 0.5 for every
    other row, which decides step 0 and scales every later score by the same exact factor; with init centers there is no start to
    choose and no weight is passed.  init: rows (host ints, in [0, N), no repeats: ValueError) that count as asked already - centers
    before the first pick, never picked.
    -> the picks as a numpy int array in pick order; shorter than n_select when the eligible rows run out."""
    return _diverse(desc, order, n_select, weighted=weighted, init=init)[0]


def _badge(desc, n_select, weight=None, init=None, seed=0, sample=True, origin=True):
    """badge_select's launch -> (picks without the -1 of an exhausted selection, picked, pick_dist, mind: the launch's tensors)"""
    if not (torch.is_tensor(desc) and desc.dim() == 2 and desc.dtype == torch.float32):
        raise ValueError('descriptors: a float32 [N, D] device tensor')
    N = int(desc.shape[0])
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError('seed: an integer in [0, 2^64)')
    if weight is not None:
        weight = np.asarray(weight, dtype=np.float32)
        if weight.shape != (N,):
            raise ValueError('weight: %d floats for %d descriptors' % (weight.size, N))
        weight = torch.from_numpy(np.ascontiguousarray(weight)).to(desc.device)
    init = None if init is None or len(init) == 0 else np.asarray(init, dtype=np.int64)
    picked, dist, mind, _ = lib.kcenter_sample(desc, n_select, weight=weight, init=init, seed=int(seed), sample=sample, origin=origin)
    picks = picked.cpu().numpy().astype(np.int64)
    return picks[picks >= 0], picked, dist, mind


def badge_select(desc, n_select, weight=None, init=None, seed=0, sample=True, origin=True):
    """batch selection in a gradient-embedding space (BADGE, Ash et al. 2020): n_select picks by k-means++ seeding - step s draws a
    row with probability proportional to its squared distance to the nearest pick so far (lib.kcenter_sample, one call).  desc:
    device f32 [N, D] (GradBank.desc, or any descriptors).  origin: the zero vector is a center before the first pick, so the first
    draw is proportional to the squared gradient length - a sample the model is certain of sits at the origin and is never drawn
    while others remain.  sample=False: greedy k-center instead of the draw (with origin: the largest gradient first).  weight: None,
    or N floats (host) that multiply the squared distances; init: rows (host ints, in [0, N), no repeats: ValueError) that count as
    asked already; seed: an int in [0, 2^64) - the same seed gives the same picks, bit for bit.  A NaN descriptor row is never picked.
    -> (sel, picked, dist, mind): sel the picks as a numpy int array in pick order, shorter than n_select when the eligible rows run
    out; picked i32 [n_select] (-1 past their end), dist f32 [n_select] and mind f32 [N] the launch's device tensors."""
    return _badge(desc, n_select, weight=weight, init=init, seed=seed, sample=sample, origin=origin)


def check_round(posterior='deterministic', bank=None, mc_samples=None, rank_by='uncert_video', observe_by='uncert_frame',
                renew_by='heuristic', acquire_by=None, soft_out=None, answer_noise=None, annotator_flip=None, questions_per_clip=1,
                stop_entropy=None, temperature=None, calibrate=None, questions_at_once=1, hit_iou=0.7, stop_hit=None, select_by=None,
                descriptors=None, diversity_init=None, selection_seed=None):
    """every rule between the switches of update_labels / run_round (their docstrings say what each switch does) -> RoundPolicy;
    raises ValueError, and touches nothing"""
    # the selection: the ranking's top half, or a diverse half of it
    if select_by not in SELECT_BY:
        raise ValueError("select_by: None, 'kcenter' or 'badge'")
    if select_by is None and descriptors is not None:
        raise ValueError("descriptors without select_by='kcenter' or 'badge': nothing reads them")
    if select_by is None and diversity_init is not None:
        raise ValueError("diversity_init without select_by='kcenter' or 'badge': nothing reads it")
    if diversity_init not in DIVERSITY_INIT:
        raise ValueError("diversity_init: None or 'answered'")
    if select_by is not None and not (torch.is_tensor(descriptors) and descriptors.dim() == 2 and descriptors.dtype == torch.float32
                                      and 1 <= descriptors.shape[1] <= lib.KCENTER_MAX_D and descriptors.shape[0] >= 1):
        raise ValueError("select_by='%s' needs descriptors: a float32 [N, D] device tensor, 1 <= D <= %d "
                         "(DeviceDataset.clip_descriptors(), GradBank.desc)" % (select_by, lib.KCENTER_MAX_D))
    if selection_seed is not None and select_by != 'badge':
        raise ValueError("selection_seed without select_by='badge': nothing draws")
    if selection_seed is not None and (isinstance(selection_seed, bool) or not isinstance(selection_seed, (int, np.integer))
                                       or not 0 <= int(selection_seed) < 1 << 64):
        raise ValueError('selection_seed: None or an integer in [0, 2^64)')
    readers = {"observe_by='info_gain'": observe_by == 'info_gain', "acquire_by='label_gain'": acquire_by == 'label_gain',
               "renew_by='posterior'": renew_by == 'posterior', 'soft_out': soft_out is not None, "rank_by='span_bald'": rank_by == 'span_bald',
               "rank_by='label_miss'": rank_by == 'label_miss', "renew_by='hit_prob'": renew_by == 'hit_prob'}

    def needs_reader(who, but):
        """`who` changes the span posterior, which is idle work unless something reads it: all of `readers` count but the one that
        `who` is not offered with"""
        if not any(on and r != but for r, on in readers.items()):
            raise ValueError('%s changes the span posterior: switch on one of its readers (%s)' % (who, ', '.join(r for r in readers if r != but)))

    def number(x, ok):
        """ok(x), False where x is no number at all"""
        try:
            return bool(ok(x))
        except (TypeError, ValueError, ZeroDivisionError):
            return False

    # the posterior: the ensemble needs its passes, has no label gain, no sessions and no evidence grid, and is the only one with span_bald
    if posterior not in POSTERIOR:
        raise ValueError("posterior: 'deterministic' or 'ensemble'")
    if posterior != 'ensemble':
        if rank_by == 'span_bald':
            raise ValueError("rank_by='span_bald' is the ensemble's score: it needs posterior='ensemble'")
    else:
        check_bank_planes(bank, mc_samples)
        if acquire_by == 'label_gain':
            raise ValueError("posterior='ensemble' with acquire_by='label_gain' is not offered: the label gain has no ensemble form")
        if questions_per_clip != 1:
            raise ValueError("posterior='ensemble' with questions_per_clip > 1 is not offered: sessions have no ensemble form")
        if calibrate is not None:
            raise ValueError("posterior='ensemble' with calibrate is not offered: the evidence grid has no ensemble form")
        if rank_by == 'label_miss' or renew_by == 'hit_prob':
            raise ValueError("posterior='ensemble' with rank_by='label_miss' or renew_by='hit_prob' is not offered: the hit probability "
                             "of a label has no ensemble form")
        needs_reader("posterior='ensemble'", but="acquire_by='label_gain'")
    # sessions: Q questions per clip, asked by information gain, stopped at stop_entropy bits
    if not number(questions_per_clip, lambda q: not isinstance(q, bool) and int(q) == q and 1 <= int(q) <= lib.AL_SESSION_MAX_Q):
        raise ValueError('questions_per_clip: an integer in [1, %d]' % lib.AL_SESSION_MAX_Q)
    Q = int(questions_per_clip)
    if Q > 1 and acquire_by == 'label_gain':
        raise ValueError("questions_per_clip > 1 with acquire_by='label_gain' is not offered: sessions ask by information gain")
    if Q > 1 and observe_by != 'info_gain':
        raise ValueError("questions_per_clip > 1 needs observe_by='info_gain': a session asks by expected information gain")
    if stop_entropy is not None and not (Q > 1 and number(stop_entropy, lambda h: float(h) >= 0.0)):
        raise ValueError('stop_entropy: None, or bits >= 0 with questions_per_clip > 1')
    if stop_hit is not None and not (Q > 1 and not isinstance(stop_hit, bool) and number(stop_hit, lambda p: 0.0 < float(p) <= 1.0)):
        raise ValueError('stop_hit: None, or a hit probability in (0, 1] with questions_per_clip > 1')
    # question sets: M frames per clip asked together, designed by information gain under the deterministic posterior
    if not number(questions_at_once, lambda q: not isinstance(q, bool) and int(q) == q and 1 <= int(q) <= lib.AL_DESIGN_MAX_M):
        raise ValueError('questions_at_once: an integer in [1, %d]' % lib.AL_DESIGN_MAX_M)
    M = int(questions_at_once)
    if M > 1 and posterior != 'deterministic':
        raise ValueError("questions_at_once > 1 with posterior='ensemble' is not offered: the design has no ensemble form")
    if M > 1 and acquire_by is not None:
        raise ValueError("questions_at_once > 1 with acquire_by='label_gain' is not offered: a design asks by information gain")
    if M > 1 and Q != 1:
        raise ValueError('questions_at_once > 1 with questions_per_clip > 1 is not offered: a clip is asked adaptively or at once')
    if M > 1 and observe_by != 'info_gain':
        raise ValueError("questions_at_once > 1 needs observe_by='info_gain': a design asks by expected information gain")
    if soft_out is not None and not isinstance(soft_out, dict):
        raise ValueError('soft_out: None or a dict to receive y1, y2, live and answered')
    # the noisy annotator, the temperature and their fit change what the posterior's readers see
    noise = None
    if answer_noise is not None:
        try:
            noise = check_noise(answer_noise)
        except ValueError:
            raise ValueError('answer_noise: None or an error probability in (0, 0.5]') from None
        needs_reader('answer_noise', but="rank_by='span_bald'")
    if calibrate not in CALIBRATE:
        raise ValueError("calibrate: None or 'evidence'")
    if temperature is not None and not number(temperature, lambda t: not isinstance(t, bool) and 0.0 < float(np.float32(1.0 / float(t))) < float('inf')):
        raise ValueError('temperature: None or a finite temperature > 0')
    if temperature is not None or calibrate is not None:
        needs_reader('calibrate' if calibrate is not None else 'temperature', but="rank_by='span_bald'")
    if annotator_flip is not None:
        if not (isinstance(annotator_flip, (tuple, list)) and len(annotator_flip) == 2 and isinstance(annotator_flip[1], np.random.Generator)
                and number(annotator_flip[0], lambda r: 0.0 <= float(r) <= 1.0)):
            raise ValueError('annotator_flip: None or (rate in [0, 1], numpy.random.Generator)')
        annotator_flip = (float(annotator_flip[0]), annotator_flip[1])
    # ranking and the question: acquire_by decides both
    if rank_by not in RANK_BY + RANK_BY_HIT + RANK_BY_GRAD and not (posterior == 'ensemble' and rank_by in RANK_BY_ENSEMBLE):
        raise ValueError("rank_by: 'uncert_video', 'span_risk', 'label_miss' or 'egl' ('span_bald' with posterior='ensemble')")
    if observe_by not in OBSERVE_BY:
        raise ValueError("observe_by: 'uncert_frame' or 'info_gain'")
    if renew_by not in RENEW_BY + RENEW_BY_HIT:
        raise ValueError("renew_by: 'heuristic', 'posterior' or 'hit_prob'")
    if isinstance(hit_iou, bool) or not number(hit_iou, lambda x: float(x) in HIT_IOUS):
        raise ValueError('hit_iou: one of 0.3, 0.5, 0.7')
    if acquire_by not in ACQUIRE_BY:
        raise ValueError("acquire_by: None or 'label_gain'")
    if acquire_by is not None and (rank_by != RANK_BY[0] or observe_by != OBSERVE_BY[0]):
        raise ValueError("acquire_by='%s' chooses the samples and the frames itself: leave rank_by and observe_by at their defaults"
                         % acquire_by)
    return RoundPolicy(posterior, rank_by, observe_by, renew_by, acquire_by, Q, None if stop_entropy is None else float(stop_entropy), noise,
                       None if temperature is None else float(temperature), calibrate, annotator_flip, any(readers.values()), M,
                       float(hit_iou), stop_hit=None if stop_hit is None else float(stop_hit), select_by=select_by, descriptors=descriptors,
                       diversity_init=diversity_init, selection_seed=None if selection_seed is None else int(selection_seed))


def grad_length(last_prop):
    """prop_egl of every record (float64 [N]): the expected squared gradient length of the localizing loss at the span heads"""
    if not all('prop_egl' in p for p in last_prop):
        raise ValueError("rank_by='egl' needs records that hold 'prop_egl': run infer_trainset(grad_bank=)")
    return np.array([float(p['prop_egl']) for p in last_prop], dtype=np.float64)


def span_risk(last_prop):
    """1 - prop_conf of every record (float64 [N]): the expected loss of temporal IoU of the record's own proposal"""
    if not all('prop_conf' in p for p in last_prop):
        raise ValueError("rank_by='span_risk' needs records that hold 'prop_conf': run infer_trainset(span_conf=True)")
    return 1.0 - np.array([float(p['prop_conf']) for p in last_prop], dtype=np.float64)


# The phases of update_labels, in its order.  Each returns what the next ones need and, last, the entries it has for the debug dict:
# device tensors as they are, fetched only if the dict is asked for.
def _round_score(pol, last_prop, aps, coff, device, bank, mc_samples, mc_stat):
    """the round's LabelUpdater, scored"""
    if bank is not None:
        up = LabelUpdater.from_bank(bank, [p['v_len'] for p in last_prop], aps, K=mc_samples, stat=mc_stat, ensemble=pol.posterior == 'ensemble')
    else:
        up = LabelUpdater(last_prop, aps, device=device)
    up.score(coff[6])
    return up, dict(uncert_frame=up.uncert_frame, sprob=up.sprob, eprob=up.eprob, updater=up)


def _round_calibrate(up, pol):
    """the temperature and error rate the round's posterior readers use: the policy's, or their fit to the answers of the earlier
    rounds where calibrate asks for it and the fit exists -> noise"""
    tau, noise, dbg = pol.temperature, pol.noise, {}
    if pol.calibrate == 'evidence':
        fit = dbg['calibration'] = up.calibrate(at_eps=noise)
        if fit is not None:
            tau, noise = fit['tau'], fit['eps']
    up.set_temperature(tau)
    return noise, dbg


def _round_choose(up, pol, noise, risk, frames, old_idx, egl=None):
    """whom to ask and where, on the answers of the earlier rounds (before set_active_points) -> (order, the ranking of the samples;
    ask, every sample's frame)"""
    uv, observe = up.uncert_video.cpu().numpy(), up.observe.cpu().numpy()
    ask, dbg = observe, dict(uncert_video=uv, observe=observe)
    order = np.argsort(uv if risk is None else risk, kind='stable')      # sorted(key=uncert_video), ties in sample order
    if risk is not None:
        dbg['span_risk'] = risk
    if egl is not None:
        order = np.argsort(-egl, kind='stable')                  # the longest expected gradient first, ties in sample order; rows at -1 last
        dbg['egl'] = egl
    if pol.observe_by == 'info_gain' or pol.rank_by == 'span_bald':
        ens = up.query(frames=frames or noise is not None, noise=noise)
        if ens is not None:
            dbg.update(weight=ens['weight'], ens_log_evidence=ens['log_evidence'], expected_entropy=ens['expected_entropy'],
                       span_bald=ens['span_bald'])
    if pol.observe_by == 'info_gain':
        ask = np.where(up.query_gain.cpu().numpy() > 0, up.query_point.cpu().numpy(), observe)
        dbg.update(query_point=up.query_point, query_gain=up.query_gain, post_entropy=up.post_entropy, observe_used=ask)
        if noise is None and up.agree is not None:               # (neither the noisy posterior nor the ensemble has an agree)
            dbg['agree'] = up.agree
    if pol.rank_by == 'span_bald':
        order = np.argsort(-up.span_bald.cpu().numpy(), kind='stable')      # largest first, ties in sample order; rows at -1 last
    if pol.rank_by == 'label_miss':                              # one candidates-only launch over the whole set: k = 1, no search
        up.hit_label(cand=np.asarray(old_idx)[:, None, :], thresholds=HIT_IOUS, best=False, noise=noise)
        old_hit = up.cand_hit.cpu().numpy()[:, 0, :]
        hit = old_hit[:, HIT_IOUS.index(pol.hit_iou)]
        miss = np.where(hit < 0, np.float32(-1.0), np.float32(1.0) - hit).astype(np.float32)      # (-1: no span of the clip, or a row without a posterior)
        order = np.argsort(-miss, kind='stable')                 # the likeliest miss first, ties in sample order; rows at -1 last
        dbg.update(label_miss=miss, old_hit=old_hit)
    if pol.acquire_by == 'label_gain':
        up.label_gain(frames=frames, noise=noise)
        ask_gain = up.ask_gain.cpu().numpy()
        ask = np.where(ask_gain > 0, up.ask_point.cpu().numpy(), observe)
        order = np.argsort(-ask_gain, kind='stable')             # largest gain first, ties in sample order; rows at 0 and -1 last
        dbg.update(ask_point=up.ask_point, ask_gain=ask_gain, label_value=up.label_value, observe_used=ask)
    dbg['order'] = order
    return order, ask, dbg


def _round_select(pol, order, aps):
    """the samples to ask, on the answers of the earlier rounds: the top half of the ranking, or under select_by='kcenter' a diverse
    half of it (diverse_select; with diversity_init='answered' around the samples that hold an active point, and filled from the
    ranking, best first, where the others run out)"""
    N = len(order)
    n_select = math.ceil(N / 2)
    if pol.select_by is None:
        return order[:n_select], {}
    init = [i for i, a in enumerate(aps) if len(a)] if pol.diversity_init == 'answered' else None
    if pol.select_by == 'badge':                                 # D^2 sampling from the origin: the descriptors carry the uncertainty themselves
        sel, picked, dist, mind = _badge(pol.descriptors, n_select, init=init, seed=pol.selection_seed or 0)
    else:
        sel, picked, dist, mind = _diverse(pol.descriptors, order, n_select, weighted=True, init=init)
    if len(sel) < n_select:
        asked = set(sel.tolist())
        sel = np.concatenate([sel, np.array([i for i in order.tolist() if i not in asked][:n_select - len(sel)], dtype=np.int64)])
    return sel, dict(kcenter_picked=picked.cpu().numpy().astype(np.int64), kcenter_dist=dist, cover_radius=float(mind.max()))


def _round_ask(up, pol, noise, sel, ask, gt_idx, data_old, aps):
    """append_AP (utils_hual.py:133-139): the annotator answers "is the observed frame inside the ground-truth span?" - up to Q times
    for a selected sample whose first question has a positive gain (one session launch for all of them), or about the M frames of
    its design at once (one design launch for all of them, answered here), once at the chosen frame for every other; the answers go
    into data_old and aps, and the updater takes the new lists"""
    N, Q, M = len(aps), pol.Q, pol.questions_at_once
    flips = np.zeros(N, dtype=np.uint32)                         # bit k: the sample's k-th answer is wrong
    if pol.flip is not None:
        rate, rng = pol.flip
        for i in sel:                                            # Q (M for a design) draws per selected sample, in selection order, used or not
            for k in range(max(Q, M)):
                if rng.random() < rate:
                    flips[i] |= np.uint32(1 << k)
    in_session = in_design = np.zeros(0, dtype=np.int64)
    if Q > 1 or M > 1:                                           # (both need observe_by='info_gain': query() ran and left query_gain)
        has_gain = up.query_gain.cpu().numpy() > 0
        in_session, in_design = (sel[has_gain[sel]], in_design) if Q > 1 else (in_session, sel[has_gain[sel]])
    if len(in_session) and pol.stop_hit is not None:             # the same sessions, stopped once the label is reliable at hit_iou
        asked, answers, n_asked = up.session_label(gt_idx, Q, thresholds=HIT_IOUS, stop_hit=pol.stop_hit, stop_at=pol.hit_iou,
                                                   stop_entropy=pol.stop_entropy, noise=noise, flips=flips, sel=in_session)
    elif len(in_session):
        asked, answers, n_asked = up.session(gt_idx, Q, stop_entropy=pol.stop_entropy, noise=noise, flips=flips, sel=in_session)
    if len(in_design):                                           # one launch for all of them; the annotator answers below, on the host
        frames, n_design = up.design(M, noise=noise, sel=in_design)
    session, ask, gt, wrong = set(in_session.tolist()), ask.tolist(), gt_idx.tolist(), flips.tolist()      # (plain lists: the loop below is per sample)
    designed = set(in_design.tolist())
    given, flipped = {}, np.zeros(N, dtype=bool)                 # given: sample -> this round's (frame, is_pos), in the order asked
    for i in sel.tolist():
        if i in session:
            given[i] = [(int(asked[i, k]), bool(answers[i, k])) for k in range(n_asked[i])]
        elif i in designed:                                      # the design's frames, answered together: draw k decides answer k
            given[i] = [(int(p), (gt[i][0] <= int(p) <= gt[i][1]) != bool((wrong[i] >> k) & 1)) for k, p in enumerate(frames[i, :n_design[i]])]
        else:                                                    # neither: the reference's or the chosen frame, one question
            given[i] = [(ask[i], (gt[i][0] <= ask[i] <= gt[i][1]) != bool(wrong[i] & 1))]
        if wrong[i] & ((1 << len(given[i])) - 1):
            flipped[i] = True
        for p, is_pos in given[i]:
            data_old[i][4]['pos_idx' if is_pos else 'neg_idx'].append(p)
            aps[i].append((p, is_pos))
    up.set_active_points(aps)
    dbg = {}
    if Q > 1:                                                    # the transcripts: -1 = unused / not read / no session
        dbg = dict(asked=np.full((N, Q), -1, dtype=np.int64), answers=np.full((N, Q), -1, dtype=np.int64), n_asked=np.zeros(N, dtype=np.int64),
                   entropy_path=np.full((N, Q + 1), -1.0, dtype=np.float32), stop_reason=np.full(N, -1, dtype=np.int64))
        for i, qa in given.items():
            dbg['asked'][i, :len(qa)], dbg['answers'][i, :len(qa)], dbg['n_asked'][i] = [p for p, _ in qa], [a for _, a in qa], len(qa)
        if len(in_session):
            dbg['entropy_path'][in_session] = up.entropy_path.cpu().numpy()[in_session]
            dbg['stop_reason'][in_session] = up.stop_reason.cpu().numpy()[in_session]
        if pol.stop_hit is not None:                             # the label trails: -1 = unused / not live / no session
            dbg.update(label_path=np.full((N, Q + 1, 2), -1, dtype=np.int32), label_conf_path=np.full((N, Q + 1), -1.0, dtype=np.float32),
                       label_hit_path=np.full((N, Q + 1, len(HIT_IOUS)), -1.0, dtype=np.float32))
            if len(in_session):
                for key in ('label_path', 'label_conf_path', 'label_hit_path'):
                    dbg[key][in_session] = getattr(up, key).cpu().numpy()[in_session]
    if M > 1:                                                    # the designs as the launch left them: -1 = unused / no design
        dbg = dict(design=np.full((N, M), -1, dtype=np.int64), design_info=np.full((N, M), -1.0, dtype=np.float32),
                   n_design=np.zeros(N, dtype=np.int64), design_stop=np.full(N, -1, dtype=np.int64))
        if len(in_design):
            dbg['design'][in_design], dbg['n_design'][in_design] = frames[in_design], n_design[in_design]
            dbg['design_info'][in_design] = up.design_info.cpu().numpy()[in_design]
            dbg['design_stop'][in_design] = up.design_stop.cpu().numpy()[in_design]
    if pol.flip is not None:
        dbg['flipped'] = flipped
    if noise is not None and pol.posterior != 'ensemble':        # (the ensemble's readers tilt the passes themselves, on demand)
        up.tilt(noise)                                           # (this round's answers included: what the launches below read)
        dbg['log_evidence'] = up.log_evidence
    return dbg


def _round_soft_labels(up, noise, aps, soft_out):
    """the whole set's soft labels under the posterior given every answer so far, into the caller's dict"""
    up.span_marginals(noise=noise)
    soft_out.update(y1=up.y_start, y2=up.y_end, live=up.marg_status.cpu().numpy() == 1,
                    answered=np.array([any(0 <= f < int(up.vlen_h[i]) for f, _ in a) for i, a in enumerate(aps)], dtype=bool))


def _round_renew(up, pol, noise, sel, old_idx, coff, data_old):
    """the selected samples' new spans - the reference's renew_label, or the minimum-Bayes-risk label (under renew_by='hit_prob'
    replaced by the span of maximal hit probability where that beats it by more than HIT_MARGIN) with that renew for the rows that
    give none - written into data_old as times"""
    dbg = {}
    if pol.renew_by in ('posterior', 'hit_prob'):
        new_idx, label_conf, old_conf = up.mbr_label(sel, old_idx, noise=noise)
        by_posterior = np.zeros(len(old_idx), dtype=bool)
        by_posterior[sel] = new_idx[sel, 0] >= 0
        dbg.update(label_conf=label_conf, old_conf=old_conf, renewed_by_posterior=by_posterior)
        if pol.renew_by == 'hit_prob':                           # one launch on the selected rows: (old label, MBR label) and the search
            up.hit_label(sel=sel, cand=np.stack([np.asarray(old_idx), new_idx], axis=1), thresholds=HIT_IOUS, noise=noise)
            hits, best_idx, best_prob = up.cand_hit.cpu().numpy(), up.hit_best_idx.cpu().numpy(), up.hit_best_prob.cpu().numpy()
            c = HIT_IOUS.index(pol.hit_iou)
            # the max-hit span only where it beats the MBR label by more than a tie: once answers shrink the consistent set many
            # members hit every remaining truth, and the search's pick among them is merely the first in row-major order
            by_hit = by_posterior & (best_prob[:, c].astype(np.float64) - hits[:, 1, c].astype(np.float64) > HIT_MARGIN)
            new_idx[by_hit] = best_idx[by_hit, c]
            dbg.update(old_hit=hits[:, 0], label_hit=hits[:, 1], hit_best_idx=best_idx, hit_best_prob=best_prob, renewed_by_hit=by_hit)
        rest = sel[~by_posterior[sel]]                           # no label: the reference's renew for just those
        if len(rest):
            new_idx[rest] = up.renew(rest, old_idx, coff)[rest]
    else:
        new_idx = up.renew(sel, old_idx, coff)
    for i in sel:
        dur, vl = data_old[i][1], int(up.vlen_h[i])
        data_old[i][2] = [round(int(t) / (vl - 1) * dur, 2) for t in new_idx[i]]          # index_to_time, update_label.py:50-57
    dbg['new_idx'] = new_idx
    return dbg


def _round_debug(*parts):
    """the debug dict of update_labels: the phases' entries, device tensors fetched"""
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for part in parts for k, v in part.items()}


def update_labels(data_old, data_gt, last_prop, coff, device='cuda:0', return_debug=False, bank=None, mc_samples=None, mc_stat='range',
                  rank_by='uncert_video', observe_by='uncert_frame', renew_by='heuristic', acquire_by=None, soft_out=None,
                  answer_noise=None, annotator_flip=None, questions_per_clip=1, stop_entropy=None, temperature=None, calibrate=None,
                  posterior='deterministic', questions_at_once=1, hit_iou=0.7, stop_hit=None, select_by=None, descriptors=None,
                  diversity_init=None, selection_seed=None):
    """update_label.main (update_label.py:173-208) without the file IO.

    data_old / data_gt: lists [vid, duration, [start_time, end_time], sentence(, active points)] as in
    data/<task>_re<I>/train.json; last_prop: the records of results/<task>/re<I-1>.pkl; coff: get_coff(task, I).
    Mutates and returns data_old exactly as the reference writes it to data/<task>_re<I>/train.json.
    bank: the McBank the K-pass inference that made last_prop folded into - the model uncertainty is then read from it on the device
    (mc_samples = its K, default bank.K; mc_stat 'range' or 'std', or 'bald', 'entropy' or 'expected_entropy' from a bank with
    info=True); last_prop then only names the samples ('vid', 'v_len').  Without a bank, records that hold 'prop_uncert' are scored from
    that recorded term, whichever statistic it is.
    rank_by: 'uncert_video' (the reference's key) or 'span_risk' - the samples are then ranked by 1 - prop_conf of their records
    (infer_trainset(span_conf=True)), the same stable argsort, the same half selected; everything else in the round is unchanged.
    observe_by: 'uncert_frame' (the reference's frame: the argmax of uncert_frame) or 'info_gain' - every selected sample is then asked
    about the frame of most expected information gain under its span posterior given the answers of the earlier rounds
    (LabelUpdater.query, one more launch; where that gain is not positive - a collapsed posterior, contradictory answers, a poisoned
    row - the reference's frame); ranking, selection, append_AP, renew and the time conversion are unchanged.
    renew_by: 'heuristic' (the reference's renew_label) or 'posterior' - every selected sample's new span is then the span of maximal
    expected temporal IoU under its span posterior given its answers, this round's included (LabelUpdater.mbr_label, one launch
    instead of the renew; the selected samples that come back without a label - contradictory answers, a poisoned row - take the
    reference's renew, one launch over just those); ranking, selection, append_AP and the time conversion are unchanged.
    acquire_by: None, or 'label_gain' - samples and frames are then both chosen by the tIoU the minimum-Bayes-risk label is expected to
    gain from the answer under the span posterior given the answers of the earlier rounds (LabelUpdater.label_gain, one more launch):
    the samples are ranked by their largest gain, descending, the same stable argsort, the same half selected, and each is asked at its
    frame of maximal gain (where that gain is not positive, the reference's frame).  It replaces the ranking and the question, so
    rank_by and observe_by must be at their defaults; append_AP, renew (either renew_by) and the time conversion are unchanged.
    soft_out: None, or a dict that receives the soft labels of the WHOLE set under the span posterior given every answer so far, this
    round's included (LabelUpdater.span_marginals, one more launch, where the renew runs; the answers earlier rounds left on samples
    that are not selected count too): 'y1', 'y2' (device f32 [N, ld], the start / end marginals), 'live' (numpy bool [N]: the row gave
    marginals) and 'answered' (numpy bool [N]: at least one active point with a frame inside [0, v_len)).  Nothing else about the call
    changes, with any combination of the other switches.
    answer_noise: None, or eps in (0, 0.5] - the span posterior then takes every answer as wrong with probability eps instead of as a
    hard constraint (LabelUpdater.tilt: one launch per state of the answers, before and after this round's), so a wrong click neither
    makes a row contradictory nor deletes the true span for good.  It is handed as noise=eps to whichever of observe_by='info_gain',
    acquire_by='label_gain', renew_by='posterior' and soft_out are on - at least one must be.  The fallbacks stay: a row that still
    gives no label (now only a poisoned one) takes the reference's route.  The debug dict gains 'log_evidence' (float32 [N]: ln P(every
    answer so far, this round's included | the model, eps)); under noise there is no 'agree'.
    annotator_flip: None, or (rate, numpy Generator) - a simulated annotator who errs: every answer of the round is flipped with
    probability rate (one draw per selected sample, in selection order) before append_AP; the debug dict gains 'flipped' (bool [N]).
    Independent of answer_noise: without it the hard rule meets the wrong answers.
    questions_per_clip: 1 (the reference's one question per selected sample: every launch and result as without the argument), or
    Q in 2..16 with observe_by='info_gain' - every selected sample whose first question has a positive gain then runs an annotation
    session on the device (LabelUpdater.session, one launch for all of them): up to Q questions, each chosen after the previous
    answer under the posterior given every answer so far (with the round's answer_noise), stopped early by a collapsed posterior, by
    contradictory answers, or by stop_entropy (None, or bits: no further question once the posterior's entropy is at most that).  A
    selected sample whose first question has no positive gain takes the reference's frame, one question, as today.  annotator_flip
    then draws Q numbers per selected sample, in selection order, used or not: draw k decides the sample's k-th answer.  Ranking,
    selection, renew (either renew_by), soft_out and the time conversion are unchanged and read the lists after the sessions;
    pos_idx / neg_idx receive the session's points in order.  The debug dict gains 'asked', 'answers' (int [N, Q], -1 = unused),
    'n_asked', 'entropy_path' (float32 [N, Q + 1], -1 = not read) and 'stop_reason' (int [N], lib.AL_STOP_REASONS; -1: no session).
    acquire_by='label_gain' sessions are not offered.  Two corners: with stop_entropy a selected sample that has a gain may already
    be at or below it before its first question - its session then asks nothing (n_asked 0, stop_reason 'entropy') and the sample gets
    no question this round.  And under answer_noise "has a positive gain" is LabelUpdater.query(noise=)'s float64 gain of the noisy
    answer, h2(eps + (1 - 2 eps) q) - h2(eps), while the kernel stops on the float32 h2(q) > 0: at the extremes of q (or eps = 0.5,
    where a noisy answer carries nothing) the two can differ; a sample the first test rejects takes the reference's frame, one the
    kernel rejects ends its session at n_asked 0 with stop_reason 'gain'.
    temperature: None, or tau > 0 - the posterior's readers (observe_by='info_gain', acquire_by='label_gain', renew_by='posterior',
    soft_out, the sessions; at least one must be on) read softmax(logits / tau) instead of the softmax itself
    (LabelUpdater.set_temperature); the reference's score and renew keep the unscaled logits.
    calibrate: None, or 'evidence' - the answers data_old already holds are fitted first (LabelUpdater.calibrate: the temperature and
    error rate of maximal evidence, three launches of hual_al_evidence_grid); where the fit exists (at least 32 answers) its tau and
    eps take the place of temperature and answer_noise for the round's posterior readers, otherwise the given values stand.  The same
    readers must be on.  The debug dict gains 'calibration' (the fit's dict, or None).  With both arguments off nothing changes.
    posterior: 'deterministic' (the span posterior of the one deterministic forward: nothing changes), or 'ensemble' - the posterior's
    readers (observe_by='info_gain', renew_by='posterior', soft_out; at least one must be on, or rank_by='span_bald') then read the
    Bayesian model average over the K stochastic passes `bank` keeps (a McBank built with passes >= K, K = mc_samples >= 1, default
    bank.K), every pass weighted by its evidence of the answers (LabelUpdater.set_ensemble: hual_al_ensemble_query /
    hual_al_ensemble_label in place of hual_al_query, hual_al_span_marginals and hual_al_mbr_label; with answer_noise behind one tilt
    per pass; temperature scales the passes too).  rank_by='span_bald' (ensemble only) ranks the samples by span_bald - the mutual
    information between the span and the dropout mask under the answers so far, bits -, largest first, the same stable argsort, the same
    half selected; rows that give none come last.  acquire_by='label_gain', questions_per_clip > 1 and calibrate have no ensemble form
    and are refused.  Under answer_noise the deterministic logits are not tilted and the debug dict has no 'log_evidence'.  The debug
    dict gains 'weight' (float32 [N, K]), 'ens_log_evidence', 'expected_entropy' and 'span_bald' (float32
    [N]) as the query left them: on the answers of the earlier rounds.
    questions_at_once: 1 (every launch and result as without the argument), or M in 2..16 with observe_by='info_gain',
    questions_per_clip=1, no acquire_by and the deterministic posterior - the annotator is then not in the loop: every selected sample
    whose first question has a positive gain (the test sessions use) is asked about up to M frames TOGETHER, the greedy design of
    most joint information under its span posterior given the answers of the earlier rounds (LabelUpdater.design, one launch for all
    of them, with the round's answer_noise and temperature; its first frame is the single question's).  The truthful annotator
    answers the design's frames on the host, as append_AP does; annotator_flip then draws M numbers per selected sample, in selection
    order, used or not: draw k decides the sample's k-th answer.  pos_idx / neg_idx receive the answers in design order; every other
    selected sample takes the reference's frame, one question; renew, soft_out and the time conversion read the lists afterwards,
    unchanged.  The debug dict gains 'design' (int [N, M], -1 = unused), 'design_info' (float32 [N, M]: the information of the first
    m + 1 frames, bits), 'n_design' and 'design_stop' (int [N], lib.AL_STOP_REASONS; -1: no design), as the launch left them: a
    sample without a design holds -1 / 0 there.  Under answer_noise the corner of the sessions applies: the kernel stops on the
    float32 h2(q) > 0, so a sample the float64 test lets in may come back with an empty design and gets no question this round.
    rank_by='label_miss' / renew_by='hit_prob' / hit_iou: label reliability (LabelUpdater.hit_label), both off by default and both
    readers of the posterior (answer_noise, temperature and calibrate are accepted with them; the ensemble has no form of them).
    hit_iou is the IoU threshold they decide at, one of 0.3, 0.5, 0.7.  rank_by='label_miss' ranks the samples by the chance that
    their CURRENT label misses: 1 - P(IoU(old label, truth) >= hit_iou) under the span posterior given the answers of the earlier
    rounds (one candidates-only launch over the whole set), largest first, the same stable argsort, the same half selected; rows
    that give no probability (-1) come last; everything else in the round is unchanged.  renew_by='hit_prob' first takes the
    minimum-Bayes-risk label as renew_by='posterior' does, then one hit_label launch on the selected rows scores the old and that
    label and searches the consistent set: the new label is the span of maximal hit probability at hit_iou only where its float32
    probability exceeds the MBR label's by more than 1e-6 (the difference taken in float64) - otherwise the MBR label stays, so the
    exact ties that are the rule once answers shrink the consistent set move no label; rows without a label take the reference's
    renew, as under 'posterior'.  It trades expected tIoU for hit probability: a different decision, not a better one.  The debug
    dict gains 'label_miss' (float32 [N]) and 'old_hit' (float32 [N, 3], columns 0.3 / 0.5 / 0.7) under the ranking, and 'old_hit',
    'label_hit' (float32 [N, 3]), 'hit_best_idx' (int32 [N, 3, 2]), 'hit_best_prob' (float32 [N, 3]) and 'renewed_by_hit' (bool [N])
    under the renew, whose 'old_hit' - this round's answers included, rows outside the selection -1 - is the one kept when both are on.
    stop_hit: None (every launch and result as without the argument), or p in (0, 1] with questions_per_clip > 1 - the sessions then
    also take, after every pass, the minimum-Bayes-risk label of the answers so far and its hit probability at hit_iou
    (LabelUpdater.session_label, one launch in place of the session's), and a session stops - stop_reason 'reliable', before the
    entropy, gain and budget rules - once that probability is at least p: "ask until the label is safe at IoU hit_iou with
    probability p".  Everything else about the sessions and the round is unchanged; the renew runs as before, so under
    renew_by='posterior' a session's final label is the label the renew gives.  The debug dict gains 'label_path' (int32 [N, Q + 1,
    2]), 'label_conf_path' (float32 [N, Q + 1]) and 'label_hit_path' (float32 [N, Q + 1, 3], columns 0.3 / 0.5 / 0.7): slot k is the
    pass before question k, slot n_asked the final label; -1 = unused, not live or no session.
    select_by: None (the top half of the ranking is asked: every launch, record and result as without the argument), or 'kcenter' -
    the asked half is then chosen as a SET: diverse_select(descriptors, order, ceil(N / 2)), greedy k-center in the descriptor space
    weighted by the ranking (lib.kcenter_select, one call), so the round's clicks are not spent on near-duplicate clips of a few
    hard videos; `order` is whatever rank_by / acquire_by made it, and everything after the selection is unchanged.  descriptors:
    device f32 [N, D], one row per sample in the order of data_old (DeviceDataset.clip_descriptors()).  diversity_init: None, or
    'answered' - the samples that already hold an active point are centers before the first pick: they count as asked, none of them
    is asked while others remain, and the picks spread around them; when fewer than ceil(N / 2) others exist the half is filled from
    the ranking, best first.  The debug dict gains 'kcenter_picked' (int [ceil(N / 2)], -1 past the end of the eligible rows),
    'kcenter_dist' (float32, the pick's squared distance to the nearest earlier center) and 'cover_radius' (float: the largest
    squared distance of any sample to its nearest asked clip).  Deterministic, so every rank of a process group gets equal picks.
    select_by='badge': the asked half is badge_select(descriptors, ceil(N / 2), seed=selection_seed or 0) - k-means++ seeding (D^2
    sampling) from the origin in the descriptor space, meant for gradient embeddings (GradBank.desc of the last infer_trainset): a
    clip is drawn with probability proportional to its squared distance to the clips drawn so far, the first to its squared
    gradient length.  The ranking takes no part in the draw; it fills the half, best first, where the eligible rows run out (a NaN
    descriptor is never drawn).  diversity_init and the three debug entries are as under 'kcenter'.  selection_seed: an int in [0,
    2^64) - the same seed gives the same half.
    rank_by='egl': the samples are ranked by 'prop_egl' of their records, largest first (infer_trainset(grad_bank=); ValueError when
    a record lacks it); the debug dict gains 'egl'.
    """
    pol = check_round(posterior=posterior, bank=bank, mc_samples=mc_samples, rank_by=rank_by, observe_by=observe_by, renew_by=renew_by,
                      acquire_by=acquire_by, soft_out=soft_out, answer_noise=answer_noise, annotator_flip=annotator_flip,
                      questions_per_clip=questions_per_clip, stop_entropy=stop_entropy, temperature=temperature, calibrate=calibrate,
                      questions_at_once=questions_at_once, hit_iou=hit_iou, stop_hit=stop_hit, select_by=select_by, descriptors=descriptors,
                      diversity_init=diversity_init, selection_seed=selection_seed)
    if pol.select_by is not None and int(pol.descriptors.shape[0]) != len(data_old):      # (raises before anything is touched)
        raise ValueError('descriptors: %d rows for %d samples' % (int(pol.descriptors.shape[0]), len(data_old)))
    risk = span_risk(last_prop) if pol.rank_by == 'span_risk' else None      # (raises before anything is touched)
    egl = grad_length(last_prop) if pol.rank_by == 'egl' else None           # (the same)
    if len(data_old[0]) == 4:
        for r in data_old:
            r.append({'pos_idx': [], 'neg_idx': []})
    N = len(data_old)
    for i in range(N):
        assert data_old[i][0] == last_prop[i]['vid'] and data_old[i][0] == data_gt[i][0]
    # active points in one list per sample; the reference keeps two lists and only ever asks for min / max / membership
    # of each, so the relative order between the two kinds does not matter
    aps = [[(f, True) for f in r[4]['pos_idx']] + [(f, False) for f in r[4]['neg_idx']] for r in data_old]
    up, scored = _round_score(pol, last_prop, aps, coff, device, bank, mc_samples, mc_stat)
    noise, fitted = _round_calibrate(up, pol)
    idx = dict(gt_idx=np.array([[_round_half_even_index(t, r[1], int(v)) for t in r[2]] for r, v in zip(data_gt, up.vlen_h)]),
               old_idx=np.array([[_round_half_even_index(t, r[1], int(v)) for t in r[2]] for r, v in zip(data_old, up.vlen_h)]))
    order, ask, chosen = _round_choose(up, pol, noise, risk, return_debug, idx['old_idx'], egl=egl)
    sel, diverse = _round_select(pol, order, aps)
    asked = _round_ask(up, pol, noise, sel, ask, idx['gt_idx'], data_old, aps)
    if soft_out is not None:
        _round_soft_labels(up, noise, aps, soft_out)
    renewed = _round_renew(up, pol, noise, sel, idx['old_idx'], coff, data_old)
    if return_debug:
        return data_old, _round_debug(scored, fitted, chosen, idx, diverse, asked, renewed)
    return data_old


# ---------------------------------------------------------------- one whole round ----------------
def labels_from_times(data, vlens):
    """pseudo-label frame indices of train.json entries: dataset_gen's time_to_index (utils/data_gen.py:98-125 ->
    data_utils.py:110-118) on every [vid, duration, [start, end], ...] record"""
    from . import data as hdata
    s, e = [], []
    for r, n in zip(data, vlens):
        a, b = hdata.time_to_index(r[2][0], r[2][1], int(n), r[1])
        s.append(a)
        e.append(b)
    return np.array(s, dtype=np.int32), np.array(e, dtype=np.int32)


def run_round(model, dataset, data_old, data_gt, last_prop, task, I, epochs, batch_size, lr, drop_rate, mc_dropout=0.5,
              shuffle_seed=0, log=None, trainer=None, mc_samples=None, mc_stat='range', bank=None, span_conf=False,
              observe_by='uncert_frame', renew_by='heuristic', acquire_by=None, soft_labels=None, answer_noise=None,
              annotator_flip=None, questions_per_clip=1, stop_entropy=None, temperature=None, calibrate=None, posterior='deterministic',
              rank_by='uncert_video', questions_at_once=1, hit_iou=0.7, stop_hit=None, select_by=None, descriptors=None,
              diversity_init=None, selection_seed=None, grad_bank=None, grad_hyp='prediction'):
    """One active-learning round of run_charades.py:9-41 on device-resident data:
         update_label.py <task> I   ->  main.py --mode train (epochs)   ->  main.py --mode infer_trainset
    dataset: DeviceDataset over the training records in the SAME order as data_old / data_gt / last_prop.
    Data parallel (torch.distributed initialised, one process per GPU): every rank calls this with the same dataset and train lists;
    `last_prop` is needed on rank 0 only (the other ranks may pass None).  Rank 0 renews the labels and broadcasts the new train
    list, the epochs run data parallel (`batch_size` clips per rank, Trainer.run_epoch), infer_trainset is sharded by batch and its
    records are gathered on rank 0.
    mc_samples=K: the round's inference runs K stochastic passes folded into a McBank (metrics['mc_bank']; `bank` if given, else a new
    one - with info=True when mc_stat is 'bald', 'entropy' or 'expected_entropy', which a given bank must have been built with).
    A `bank` that already holds the passes behind last_prop (the previous round's metrics['mc_bank']) feeds this round's label
    update on the device before it is refilled; otherwise last_prop's own 'prop_uncert' or 'prop_logits1/2' do.
    span_conf=True: the round's inference records 'prop_conf' / 'prop_span_entropy' (infer_trainset).
    observe_by: the frame the round's label update asks the annotator about (update_labels).
    renew_by: how the round's label update derives the new pseudo-labels (update_labels).
    acquire_by: how the round's label update chooses the samples and frames it asks about (update_labels).
    answer_noise / annotator_flip: the error probability the round's span posterior grants the annotator, and a simulated annotator
    who errs (update_labels).
    questions_per_clip / stop_entropy: the questions a selected sample may be asked in the round, as one session on the device, and the
    posterior entropy at which a session stops (update_labels); with more than one, metrics['sessions'] holds the transcripts (asked,
    answers, n_asked, entropy_path, stop_reason).
    questions_at_once: the frames a selected sample is asked TOGETHER in the round, designed in one launch on the device and answered on
    the host (update_labels); with more than one, metrics['designs'] holds them (design, design_info, n_design, design_stop).
    temperature / calibrate: the temperature of the round's span posterior, and its fit - with the annotator's error rate - to the
    answers of the earlier rounds by their evidence (update_labels); metrics['calibration'] holds the fit under calibrate.
    posterior / rank_by: 'ensemble' reads the round's span posterior as the model average over the passes `bank` holds from the
    PREVIOUS round's inference (update_labels), and rank_by='span_bald' ranks the samples by it.  It needs such a bank: build
    McBank.for_dataset(dataset, passes=K) once, hand it with mc_samples=K to a first round under the default posterior (or to
    infer_trainset), which fills it, and to every later round with posterior='ensemble'; without a filled bank that keeps its passes
    the call raises ValueError before anything is touched.
    rank_by='label_miss' / renew_by='hit_prob' / hit_iou: rank the samples by the chance that their current label misses at IoU
    hit_iou, and renew by the span of maximal hit probability where it beats the minimum-Bayes-risk label (update_labels).
    stop_hit: the hit probability of the label at hit_iou at which a session stops (update_labels); metrics['sessions'] then also
    holds label_path, label_conf_path and label_hit_path.
    select_by / descriptors / diversity_init: 'kcenter' asks a diverse half of the ranking instead of its top half (update_labels);
    the descriptors default to dataset.clip_descriptors(), computed once per call; metrics['diversity'] then holds kcenter_picked,
    kcenter_dist and cover_radius.  select_by='badge' (with selection_seed) draws the half by D^2 sampling instead and needs
    descriptors=: the desc of the GradBank the round before returned.
    grad_bank: None, True or a GradBank - the round's inference then fills it (True: a GradBank.for_dataset of this call), one
    hual_al_grad_embed launch per batch under the hypothesis grad_hyp (infer_trainset), the records gain 'prop_egl' / 'prop_gnorm2'
    (rank_by='egl' of the next round), and metrics['grad_bank'] is the bank: the next round passes descriptors=bank.desc.  Single
    process only.
    soft_labels: None, or a weight lam in (0, 1] - the epochs then train every sample that has an answer and a live posterior on the
    blend (weight lam) of the reference's labels with the posterior's start / end marginals (update_labels(soft_out=),
    DeviceDataset.set_soft_labels); every other sample keeps weight 0 - a clip nobody has answered about would only be trained on the
    model's own prediction.  metrics['soft_rows'] is the number of weighted samples.  Single process only (the marginals live on
    rank 0), and the records' v_len must be the dataset's clip lengths.
    Returns (new train list, new results records - rank 0 only, else None -, metrics dict)."""
    import time
    from . import dist as hdist
    from .train import Trainer
    world, rank = hdist.world_size(), hdist.rank()
    soft = None
    if soft_labels is not None:                                  # (raises before anything is touched)
        lam = float(soft_labels)
        if not 0.0 < lam <= 1.0:
            raise ValueError('soft_labels: None or a weight in (0, 1]')
        if world > 1:
            raise ValueError('soft_labels is single-process: the marginals live on rank 0 and are not broadcast')
        if [int(p['v_len']) for p in last_prop] != [int(n) for n in dataset.vlen_h]:
            raise ValueError("soft_labels: a record's v_len differs from the dataset's clip length")
        soft = {}
    t0 = time.perf_counter()
    prev = bank if bank is not None and bank.K >= (1 if posterior == 'ensemble' else 2) else None
    switches = dict(posterior=posterior, bank=prev, rank_by=rank_by, observe_by=observe_by, renew_by=renew_by, acquire_by=acquire_by,
                    soft_out=soft, answer_noise=answer_noise, annotator_flip=annotator_flip, questions_per_clip=questions_per_clip,
                    stop_entropy=stop_entropy, temperature=temperature, calibrate=calibrate, questions_at_once=questions_at_once,
                    hit_iou=hit_iou, stop_hit=stop_hit)
    if select_by is not None or descriptors is not None or diversity_init is not None:      # (a round without them: the call it was)
        if select_by == 'kcenter' and descriptors is None:
            descriptors = dataset.clip_descriptors()
        switches.update(select_by=select_by, descriptors=descriptors, diversity_init=diversity_init)
    if selection_seed is not None:
        switches.update(selection_seed=selection_seed)
    if grad_bank is not None and grad_bank is not False:
        if world > 1:
            raise ValueError('grad_bank is single-process: the rows of other ranks are not gathered')
        if grad_hyp not in GRAD_HYP:
            raise ValueError("grad_hyp: 'prediction' or 'pseudo'")
        if grad_bank is not True and not (isinstance(grad_bank, GradBank) and grad_bank.N == len(dataset)):
            raise ValueError('grad_bank: None, True or a GradBank over the dataset')
    else:
        grad_bank = None
    pol = check_round(**switches)                                # (on every rank, before rank 0 goes its own way)
    want_debug = pol.Q > 1 or pol.questions_at_once > 1 or calibrate is not None or pol.select_by is not None
    new_data = sessions = designs = calibration = diversity = None
    if rank == 0:
        new_data = update_labels(data_old, data_gt, last_prop, get_coff(task, I), device=model.device, mc_stat=mc_stat,
                                 return_debug=want_debug, **switches)
        if want_debug:
            new_data, dbg = new_data
            calibration = dbg.get('calibration')
        if pol.Q > 1:
            sessions = {k: dbg[k] for k in ('asked', 'answers', 'n_asked', 'entropy_path', 'stop_reason')
                        + (('label_path', 'label_conf_path', 'label_hit_path') if pol.stop_hit is not None else ())}
        if pol.questions_at_once > 1:
            designs = {k: dbg[k] for k in ('design', 'design_info', 'n_design', 'design_stop')}
        if pol.select_by is not None:
            diversity = {k: dbg[k] for k in ('kcenter_picked', 'kcenter_dist', 'cover_radius')}
    new_data = hdist.broadcast_object(new_data)
    if soft is not None:
        weighted = soft['live'] & soft['answered']
        dataset.set_soft_labels(soft['y1'], soft['y2'], np.where(weighted, np.float32(lam), np.float32(0.0)))
    else:
        dataset.clear_soft_labels()                              # (banks an earlier round enabled describe the labels before this update)
    torch.cuda.synchronize()
    t1a = time.perf_counter()
    # the pseudo-label frame indices of the new train list: the reference regenerates its dataset cache for this (dataset_gen,
    # utils/data_gen.py:98-125 - one time_to_index per record, a T x T overlap table each), outside its training loop
    s_ind, e_ind = labels_from_times(new_data, dataset.vlen_h)
    dataset.set_labels(s_ind, e_ind)
    for r, a, b in zip(dataset.records, s_ind, e_ind):
        r['s_ind'], r['e_ind'] = int(a), int(b)
    t1 = time.perf_counter()
    N = len(dataset)
    tr = trainer if trainer is not None else Trainer(model, world=world, use_graph=True)
    rng = np.random.default_rng(shuffle_seed)                   # the same permutations on every rank
    steps = 0
    for ep in range(epochs):
        cur_lr = lr * (1.0 - ep / epochs)                       # main.py:61
        order = rng.permutation(N)                              # random.shuffle(self.dataset), data_loader.py:24
        tr.run_epoch(dataset, order, batch_size, lr=cur_lr, drop_rate=drop_rate, min_chars=4)      # spans fetched: train_epoch's IoU log
        steps += (N + batch_size * world - 1) // (batch_size * world)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if mc_samples is not None and bank is None:
        bank = McBank.for_dataset(dataset, device=model.device, info=mc_stat in lib.AL_STAT_INFO)
    grad = {}                                                    # (a round without the bank: the call it was)
    if grad_bank is not None:
        grad_bank = GradBank.for_dataset(dataset, device=model.device) if grad_bank is True else grad_bank
        grad = dict(grad_bank=grad_bank, grad_hyp=grad_hyp)
    records, ious = infer_trainset_sharded(model, dataset, batch_size, mc_dropout=mc_dropout, min_chars=4, mc_samples=mc_samples,
                                           bank=bank if mc_samples is not None else None, mc_stat=mc_stat, span_conf=span_conf,
                                           **grad)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    met = hdist.broadcast_object(iou_metrics(ious) if rank == 0 else None)
    r3, r5, r7, mi = met
    m = dict(update_s=t1a - t0, relabel_s=t1 - t1a, train_s=t2 - t1, infer_s=t3 - t2, train_steps=steps, clips_per_s=N * epochs / max(t2 - t1, 1e-9),
             step_launch_modes=dict(tr.stats), world=world,
             r1i3=r3, r1i5=r5, r1i7=r7, miou=mi)
    if mc_samples is not None:
        m['mc_bank'] = bank
    if soft is not None:
        m['soft_rows'] = int(weighted.sum())
    if sessions is not None:
        m['sessions'] = sessions
    if designs is not None:
        m['designs'] = designs
    if calibrate is not None:
        m['calibration'] = calibration
    if diversity is not None:
        m['diversity'] = diversity
    if grad_bank is not None:
        m['grad_bank'] = grad_bank
    if log and rank == 0:
        log('round %d: update_label %.3f s | train %d steps %.3f s (%.0f clips/s) | infer_trainset %.3f s | pseudo-label '
            'R1@0.5 %.2f mIoU %.2f' % (I, m['update_s'], steps, m['train_s'], m['clips_per_s'], m['infer_s'], r5, mi))
    return new_data, records, m
