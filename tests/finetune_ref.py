"""CPU reference of a training step with a TRAINABLE word table (modules.py:8-16 with finetune=True), built only from the oracle:
oracle.forward with the GloVe matrix as a leaf that requires grad, oracle.clip_by_global_norm over every parameter gradient plus the
table's (the norm of the summed, dense gradient - the convention the oracle already uses for unk and char_table), and
oracle.adam_weight_decay_step, where uses_weight_decay('word_embs/word_table') gives the table weight decay.

Parameter / slot dicts hold the table under its TF name WORD_TABLE beside the other variables."""
import collections

import torch

from oracle import seqpan_ref as R

WORD_TABLE = 'word_embs/word_table'


def grads(p, cfg, batch, labels, drop_rate=0.0, seed=0, offset=0, relu_pin=None, want_tap=False, dtype=torch.float32):
    """oracle forward + tf.gradients over every variable incl. the table: (out, OrderedDict name -> gradient)"""
    pr = collections.OrderedDict((k, t.detach().clone().to(dtype).requires_grad_(True)) for k, t in p.items())
    model_p = collections.OrderedDict((k, t) for k, t in pr.items() if k != WORD_TABLE)
    video, lens, word_ids, char_ids = batch
    lab = tuple(x.to(dtype) if x.dtype.is_floating_point else x for x in labels)
    out = R.forward(model_p, cfg, pr[WORD_TABLE], video.to(dtype), lens, word_ids, char_ids, drop_rate=drop_rate, seed=seed,
                    offset=offset, labels=lab, relu_pin=relu_pin, want_tap=want_tap)
    names = list(pr.keys())
    gl = torch.autograd.grad(out['loss'], [pr[k] for k in names], allow_unused=True)
    g = collections.OrderedDict((k, (x if x is not None else torch.zeros_like(pr[k])).detach()) for k, x in zip(names, gl))
    return out, g


def train_step(p, m, v, cfg, batch, labels, lr, drop_rate, seed=0, offset=0, relu_pin=None, want_tap=False):
    """one sess.run([train_op, ...]) of a fine-tuning model: returns (p, m, v, info) with NEW dicts (the inputs are untouched)"""
    out, g = grads(p, cfg, batch, labels, drop_rate, seed, offset, relu_pin, want_tap)
    g, gn = R.clip_by_global_norm(g, cfg.clip_norm)
    with torch.no_grad():
        p2, m2, v2 = R.adam_weight_decay_step(collections.OrderedDict((k, t.detach()) for k, t in p.items()), g, m, v, lr)
    return p2, m2, v2, dict(loss=out['loss'].detach(), start_index=out['start_index'], end_index=out['end_index'], grad_norm=gn,
                            grads=g, tap=out.get('tap'), start_logits=out['start_logits'].detach(),
                            end_logits=out['end_logits'].detach())


def with_table(p, wv):
    """the oracle's parameter dict plus the GloVe matrix as the table entry"""
    q = collections.OrderedDict((k, t.detach().clone()) for k, t in p.items())
    q[WORD_TABLE] = wv.detach().clone()
    return q
