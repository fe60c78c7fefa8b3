"""Controlled generation: caption a video under chosen POS templates.

The captioner is steered by the global POS vector ``pos_feats`` (caption_src/data_io.py:215-217: the last state of the POS
generator's rollout).  ``PosModel.sample_forced`` rolls the POS generator along a caller's tag sequence instead of its own greedy
choice (include/xgate_pos_control.h), S templates for each of B videos; ``caption_with_templates`` feeds the resulting states to the
captioner without leaving the device.  ``PosModel.sample_templates`` (include/xgate_pos_sample.h) lets the generator draw the templates
itself, ``caption_sampled`` captions under them and ``first_occurrences`` marks a video's distinct draws.
``PosModel.beam_templates`` (include/xgate_pos_beam.h) finds the W templates the generator thinks most likely and ``caption_beam``
captions under them.  Eval mode, fp32, one GPU.  By default the captioner runs over the B*S rows with the video inputs repeated per
template; ``share_encoder=True`` hands the videos over once (``SAModel.sample_per_video``, include/xgate_control.h): the captioner's
encoder, init_hidden and v2a(V) then run once per video and a step's attention reads them once per group of a video's templates.
``beam_captions_with_templates`` is the captioner's BEAM SEARCH under the templates on one encoder pass
(``SAModel.beam_captions_per_video``, include/xgate_beam_control.h); ``caption_truncated_with_templates`` is the SAMPLED rollout
under them with top-k / nucleus truncation (``SAModel.sample_truncated_per_video``, include/xgate_truncate.h).  All of that steers; ``beam_captions_following_templates``
GUARANTEES: the same search admitting at position t only words whose POS category the template allows there
(``SAModel.beam_captions_allowed``, include/xgate_beam_allow.h; ``allow_masks`` builds the sets, ``template_adherence`` checks a result).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def _is_seq(x):
    return isinstance(x, (list, tuple))


def pad_templates(templates, seq_length, category_size):
    """POS templates as the (B,S,L) int64 tensor `PosModel.sample_forced` takes, L = seq_length, padded with 0 (the end tag).

    `templates`: nested lists ``[video][template][tag]`` (ragged in the last level; ``[video][tag]`` means one template per video)
    or an integer array / tensor (B,S,L') or (B,L') with L' <= L.  Raises ValueError for a template longer than L, a video with
    another number of templates than the first, and a tag outside [0, category_size).  A tensor that already lives on the GPU is
    padded there and its tags are NOT read (that would synchronise): the kernel clamps them into range."""
    L, Cn = int(seq_length), int(category_size)
    if _is_seq(templates):
        rows = list(templates)
        if not rows:
            raise ValueError("no templates")
        if not any(_is_seq(v) for r in rows for v in r):
            rows = [[r] for r in rows]                      # [video][tag]: one template per video
        S = len(rows[0])
        if S < 1:
            raise ValueError("every video needs at least one template")
        out = np.zeros((len(rows), S, L), dtype=np.int64)
        for b, r in enumerate(rows):
            if len(r) != S:
                raise ValueError("video %d has %d templates, video 0 has %d" % (b, len(r), S))
            for s, tags in enumerate(r):
                if len(tags) > L:
                    raise ValueError("template %d of video %d has %d tags, seq_length is %d" % (s, b, len(tags), L))
                out[b, s, :len(tags)] = np.asarray(tags, dtype=np.int64)
        t = torch.from_numpy(out)
    else:
        t = torch.as_tensor(templates)
        if t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError("templates are integer tags")
        if t.dim() == 2:
            t = t.unsqueeze(1)
        if t.dim() != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("templates (B,S,L') or (B,L') expected, got %s" % (tuple(t.shape),))
        if t.shape[2] > L:
            raise ValueError("templates have %d tags, seq_length is %d" % (t.shape[2], L))
        t = F.pad(t.long(), (0, L - t.shape[2]))
    if not t.is_cuda and t.numel() and (int(t.min()) < 0 or int(t.max()) >= Cn):
        raise ValueError("tags must lie in [0, %d)" % Cn)
    return t.contiguous()


def _caption_rows(cap_model, feats_rgb, feats_opfl, feat_mask, pos_feats, B, S, opt, share_encoder):
    """The captioner over the (B*S,R) `pos_feats` rows of B videos: (seq (B,S,n), seqLogprobs (B,S,n)).  share_encoder: the videos
    once through ``sample_per_video``; otherwise ``sample`` on the inputs repeated per template."""
    if share_encoder:
        return cap_model.sample_per_video(feats_rgb, feats_opfl, feat_mask, pos_feats.reshape(B, S, -1), opt)
    seq, slp = cap_model.sample(feats_rgb.repeat_interleave(S, 0), feats_opfl.repeat_interleave(S, 0),
                                feat_mask.repeat_interleave(S, 0), pos_feats, opt)
    return seq.reshape(B, S, -1), slp.reshape(B, S, -1)


def caption_with_templates(pos_model, cap_model, feats_rgb, feats_opfl, feat_mask, templates, opt={}, share_encoder=False):
    """Caption each of the B videos under each of its S POS templates: (seq (B,S,n) int64, seqLogprobs (B,S,n), template_score
    (B,S)).  The forced POS rollout (``pos_model.sample_forced``) leaves `pos_feats` (B*S,R) on the device and the captioner's
    ``sample`` (``opt`` as there: greedy, sampled, or beam search with beam_size > 1) runs over the B*S rows, the video inputs
    repeated per template; nothing is read back between the two.  template_score is the log-probability the POS generator gives
    the template (end tag included).  Inference only: both models run under ``torch.no_grad()``, so nothing returned carries a
    gradient (a sampled captioner rollout that is to be trained on goes through ``cap_model.sample`` directly).
    ``share_encoder=True``: the captioner takes the B videos once (``cap_model.sample_per_video``; greedy or sampled, no beam search:
    beam_size > 1 raises NotImplementedError) instead of the repeated inputs; the two paths agree up to the last bits of fp32."""
    if share_encoder and opt.get("beam_size", 1) > 1:
        raise NotImplementedError("share_encoder=True has no beam search: beam_size must be 1 (beam_captions_with_templates "
                                  "is the beam search on one encoder pass)")
    with torch.no_grad():
        tag_logp, _, _, pos_feats = pos_model.sample_forced(feats_rgb, feats_opfl, feat_mask, templates, collect_states=False,
                                                            trim=False)
        B, S = tag_logp.shape[:2]
        seq, slp = _caption_rows(cap_model, feats_rgb, feats_opfl, feat_mask, pos_feats, B, S, opt, share_encoder)
    return seq, slp, tag_logp.sum(2)


def caption_truncated_with_templates(pos_model, cap_model, feats_rgb, feats_opfl, feat_mask, templates, top_k=0, top_p=1.0,
                                     temperature=1.0, uniforms=None, return_stats=False):
    """``caption_with_templates`` with TOP-K / NUCLEUS sampling on one captioner encoder pass: (seq (B,S,n) int64, seqLogprobs
    (B,S,n), template_score (B,S)), and with ``return_stats=True`` seq_logq (B,S,n) and kept (B,S,n) int32 after them.  The forced
    POS rollout (``pos_model.sample_forced``) leaves `pos_feats` (B*S,R) on the device and
    ``cap_model.sample_truncated_per_video`` (include/xgate_truncate.h; `top_k`, `top_p`, `temperature`, `uniforms` (L + 1, B*S)
    and the statistics as there) takes the B videos once; nothing is read back between the two.  Inference only: both models run
    under ``torch.no_grad()``."""
    with torch.no_grad():
        tag_logp, _, _, pos_feats = pos_model.sample_forced(feats_rgb, feats_opfl, feat_mask, templates, collect_states=False,
                                                            trim=False)
        B, S = tag_logp.shape[:2]
        out = cap_model.sample_truncated_per_video(feats_rgb, feats_opfl, feat_mask, pos_feats.reshape(B, S, -1), top_k=top_k,
                                                   top_p=top_p, temperature=temperature, uniforms=uniforms,
                                                   return_stats=return_stats)
    return out[:2] + (tag_logp.sum(2),) + out[2:]


def beam_captions_with_templates(pos_model, cap_model, feats_rgb, feats_opfl, feat_mask, templates, beam_size=5, suppress_token=1):
    """The W = beam_size most likely captions of each of the B videos under each of its S POS templates, on one captioner encoder
    pass: (seq (B,S,W,L) int64, seq_logp (B,S,W,L), score (B,S,W), template_score (B,S)).  The forced POS rollout
    (``pos_model.sample_forced``) leaves `pos_feats` (B*S,R) on the device and ``cap_model.beam_captions_per_video``
    (include/xgate_beam_control.h; `beam_size`, `suppress_token` and the order of a pair's beams as there) takes the B videos once;
    nothing is read back between the two or after them.  `templates` as in ``caption_with_templates``: those of
    ``pos_model.sample_templates`` or ``beam_templates`` are valid inputs.  Inference only: both models run under
    ``torch.no_grad()``."""
    with torch.no_grad():
        tag_logp, _, _, pos_feats = pos_model.sample_forced(feats_rgb, feats_opfl, feat_mask, templates, collect_states=False,
                                                            trim=False)
        B, S = tag_logp.shape[:2]
        seq, seq_logp, score = cap_model.beam_captions_per_video(feats_rgb, feats_opfl, feat_mask, pos_feats.reshape(B, S, -1),
                                                                 beam_size=beam_size, suppress_token=suppress_token)
    return seq, seq_logp, score, tag_logp.sum(2)


def diverse_beam_captions_with_templates(pos_model, cap_model, feats_rgb, feats_opfl, feat_mask, templates, groups, group_size,
                                         diversity=0.5, suppress_token=1):
    """``beam_captions_with_templates`` with the diverse search: per (video, template) pair Gd = groups beam searches of width
    Wg = group_size that are steered apart (``cap_model.beam_captions_diverse``, include/xgate_beam_diverse.h; `groups`,
    `group_size`, `diversity`, `suppress_token` and the order of a group's beams as there): (seq (B,S,Gd,Wg,L) int64, seq_logp
    (B,S,Gd,Wg,L), score (B,S,Gd,Wg), template_score (B,S)).  The forced POS rollout leaves `pos_feats` on the device and the
    captioner takes the B videos once; nothing is read back between the two or after them.  Inference only: both models run under
    ``torch.no_grad()``."""
    with torch.no_grad():
        tag_logp, _, _, pos_feats = pos_model.sample_forced(feats_rgb, feats_opfl, feat_mask, templates, collect_states=False,
                                                            trim=False)
        B, S = tag_logp.shape[:2]
        seq, seq_logp, score = cap_model.beam_captions_diverse(feats_rgb, feats_opfl, feat_mask, pos_feats.reshape(B, S, -1),
                                                               groups, group_size, diversity=diversity, suppress_token=suppress_token)
    return seq, seq_logp, score, tag_logp.sum(2)


ANY_WORD = 0xFFFFFFFF                       # the mask that admits every category


def _mask_of(tag):
    """One position of a nested-list constraint: a tag, or -1 (any word)."""
    c = int(tag)
    if not -1 <= c < 32:
        raise ValueError("tags must lie in [-1, 32), got %d" % c)
    return ANY_WORD if c < 0 else 1 << c


def allow_masks(constraints, seq_length, built=False):
    """Per-position sets of admitted POS categories as the (B,S,L) int64 tensor of uint32 masks ``SAModel.beam_captions_allowed``
    takes, L = seq_length (include/xgate_beam_allow.h: bit c set = category c admitted).

    `constraints`: integer tags (B,S,L') or (B,L'), L' <= L, as an array / tensor or as nested lists ``[video][template][tag]``
    (ragged in the last level; ``[video][tag]``: one template per video).  A tag c becomes ``1 << c`` and -1 becomes 0xFFFFFFFF (any
    word).  Positions behind the last one are padded with tag 0's mask, 1: only words of the end category.  ``built=True``:
    `constraints` already holds masks, (B,S,L) integers -- the way to a set of several categories ("noun or adjective": two
    bits) --; it passes through as int64.  Raises ValueError for L' > L, a video with another number of templates than the
    first, and a tag outside [-1, 32).  A tensor that already lives on the GPU is converted there and its tags are NOT read (that
    would synchronise): they are taken modulo 32, negative ones as -1."""
    L = int(seq_length)
    if built:
        t = torch.as_tensor(constraints)
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError("masks are integers")
        if t.dim() != 3 or t.shape[2] != L:
            raise ValueError("masks (B,S,L = %d) expected, got %s" % (L, tuple(t.shape)))
        return t.long().contiguous()
    if _is_seq(constraints):
        rows = list(constraints)
        if not rows:
            raise ValueError("no constraints")
        if not any(_is_seq(v) for r in rows for v in r):
            rows = [[r] for r in rows]                      # [video][tag]: one template per video
        S = len(rows[0])
        if S < 1:
            raise ValueError("every video needs at least one template")
        out = np.ones((len(rows), S, L), dtype=np.int64)
        for b, r in enumerate(rows):
            if len(r) != S:
                raise ValueError("video %d has %d templates, video 0 has %d" % (b, len(r), S))
            for s, tags in enumerate(r):
                if len(tags) > L:
                    raise ValueError("template %d of video %d has %d tags, seq_length is %d" % (s, b, len(tags), L))
                out[b, s, :len(tags)] = [_mask_of(e) for e in tags]
        return torch.from_numpy(out)
    t = torch.as_tensor(constraints)
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError("constraints are integer tags")
    if t.dim() == 2:
        t = t.unsqueeze(1)
    if t.dim() != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("constraints (B,S,L') or (B,L') expected, got %s" % (tuple(t.shape),))
    if t.shape[2] > L:
        raise ValueError("constraints have %d tags, seq_length is %d" % (t.shape[2], L))
    t = t.long()
    if not t.is_cuda and t.numel() and (int(t.min()) < -1 or int(t.max()) >= 32):
        raise ValueError("tags must lie in [-1, 32)")
    m = torch.where(t < 0, torch.full_like(t, ANY_WORD), torch.ones_like(t) << (t & 31))
    return F.pad(m, (0, L - t.shape[2]), value=1).contiguous()


def beam_captions_following_templates(pos_model, cap_model, feats_rgb, feats_opfl, feat_mask, templates, word_cat, constraints=None,
                                      beam_size=5, suppress_token=1, built=False):
    """``beam_captions_with_templates`` with the hard guarantee: (seq (B,S,W,L) int64, seq_logp (B,S,W,L), score (B,S,W),
    template_score (B,S)).  The forced POS rollout (``pos_model.sample_forced``) gives the soft guidance `pos_feats` as before; then
    ``cap_model.beam_captions_allowed`` (include/xgate_beam_allow.h) admits at position t of a (video, template) pair's captions only
    words whose category -- `word_cat` (V,) uint8 on the device, ``data.word_category_table`` -- the pair's constraint allows at t.
    `constraints` as ``allow_masks`` takes them (`built` as there); None: the templates themselves, so every caption with a score
    above -500 has exactly its template's tag sequence and length (given that word 0 alone has category 0).  Nothing is read back
    between the two calls or after them.  Inference only: both models run under ``torch.no_grad()``."""
    with torch.no_grad():
        tag_logp, _, _, pos_feats = pos_model.sample_forced(feats_rgb, feats_opfl, feat_mask, templates, collect_states=False,
                                                            trim=False)
        B, S, L = tag_logp.shape
        allow = allow_masks(templates if constraints is None else constraints, L, built=built and constraints is not None)
        seq, seq_logp, score = cap_model.beam_captions_allowed(feats_rgb, feats_opfl, feat_mask, pos_feats.reshape(B, S, -1), word_cat,
                                                               allow.to(pos_feats.device), beam_size=beam_size,
                                                               suppress_token=suppress_token)
    return seq, seq_logp, score, tag_logp.sum(2)


def template_adherence(seq, allow, word_cat):
    """(B,S,W) bool for captions seq (B,S,W,L), masks allow (B,S,L) and the table word_cat (V,): True where every token up to and
    including the caption's first 0 (all L when it has none) is allowed at its position, by the rule of include/xgate_beam_allow.h
    -- a mask that admits no word of the table counts as 0xFFFFFFFF.  Torch ops on `seq`'s device; nothing is read back."""
    seq = torch.as_tensor(seq)
    dev = seq.device
    allow, cat = torch.as_tensor(allow).to(dev).long() & ANY_WORD, torch.as_tensor(word_cat).to(dev).long() & 31
    if seq.dim() != 4 or allow.dim() != 3 or cat.dim() != 1 or allow.shape != seq.shape[:2] + seq.shape[3:]:
        raise ValueError("seq (B,S,W,L), allow (B,S,L) and word_cat (V,) expected, got %s, %s, %s"
                         % (tuple(seq.shape), tuple(allow.shape), tuple(cat.shape)))
    present = ((torch.bincount(cat, minlength=32) > 0).long() << torch.arange(32, device=dev)).sum()
    allow = torch.where((allow & present) == 0, torch.full_like(allow, ANY_WORD), allow)
    ok = ((allow.unsqueeze(2) >> cat[seq.long()]) & 1).bool()
    open_ = (seq != 0).long().cumprod(3).bool()
    counted = torch.cat([torch.ones_like(open_[..., :1]), open_[..., :-1]], 3)
    return (ok | ~counted).all(3)


def length_scale_table(seq_length, alpha, kind="avg"):
    """The (L,) float32 `length_scale` of ``SAModel.beam_captions_ruled`` (include/xgate_beam_rules.h): entry t scales the score of
    a beam that finishes at step t, i.e. one of t + 1 tokens with its end token.  kind "avg": (t + 1) ** -alpha (alpha = 1: the
    mean log-probability per token); kind "wu": ((5 + t + 1) / 6) ** -alpha (the GNMT length penalty).  Computed in float64 and
    rounded once to fp32; every entry lies in (0, 1].  alpha >= 0; alpha = 0 gives all ones."""
    L, alpha = int(seq_length), float(alpha)
    if L < 1:
        raise ValueError("seq_length >= 1 expected, got %d" % L)
    if not (0.0 <= alpha < float("inf")):
        raise ValueError("alpha must be finite and >= 0, got %r" % (alpha,))
    n = np.arange(1, L + 1, dtype=np.float64)
    if kind == "avg":
        base = n
    elif kind == "wu":
        base = (5.0 + n) / 6.0
    else:
        raise ValueError("kind 'avg' or 'wu' expected, got %r" % (kind,))
    return torch.from_numpy(np.power(base, -alpha).astype(np.float32))


def repeated_ngrams(seq, n):
    """(..) bool for captions seq (.., L): True where the caption's words -- its tokens before the first 0, all L when it has none
    -- hold the same n-gram at two different positions.  Torch ops on `seq`'s device; nothing is read back."""
    seq, n = torch.as_tensor(seq), int(n)
    if n < 1:
        raise ValueError("n >= 1 expected, got %d" % n)
    if seq.dim() < 1 or seq.is_floating_point():
        raise ValueError("seq (.., L) integer tokens expected")
    L = seq.shape[-1]
    if n >= L:                                       # at most one n-gram
        return torch.zeros(seq.shape[:-1], dtype=torch.bool, device=seq.device)
    words = (seq != 0).long().cumprod(-1).sum(-1)                                   # (..)
    g = seq.unfold(-1, n, 1)                                                        # (.., L-n+1, n)
    P = g.shape[-2]
    valid = torch.arange(P, device=seq.device) + n <= words.unsqueeze(-1)           # (.., P): the n-gram lies inside the words
    same = (g.unsqueeze(-2) == g.unsqueeze(-3)).all(-1)                             # (.., P, P)
    later = torch.ones(P, P, dtype=torch.bool, device=seq.device).triu(1)
    return (same & later & valid.unsqueeze(-1) & valid.unsqueeze(-2)).flatten(-2).any(-1)


def beam_captions_ruled_with_templates(pos_model, cap_model, feats_rgb, feats_opfl, feat_mask, templates, word_cat=None,
                                       constraints=None, built=False, **rules):
    """``beam_captions_with_templates`` -- with `word_cat`, ``beam_captions_following_templates`` -- under decoding rules: (seq
    (B,S,W,L) int64, seq_logp (B,S,W,L), score (B,S,W), key (B,S,W), template_score (B,S)).  The forced POS rollout
    (``pos_model.sample_forced``) leaves `pos_feats` on the device and ``cap_model.beam_captions_ruled``
    (include/xgate_beam_rules.h) takes the B videos once; `rules` are that method's keywords (beam_size, suppress_token,
    no_repeat_ngram, min_length, bad_endings, length_scale).  `word_cat` (V,) uint8 on the device turns the hard template
    constraint on: `constraints` and `built` as ``beam_captions_following_templates`` takes them, None: the templates themselves.
    Inference only: both models run under ``torch.no_grad()``."""
    if word_cat is None and constraints is not None:
        raise ValueError("constraints need word_cat")
    with torch.no_grad():
        tag_logp, _, _, pos_feats = pos_model.sample_forced(feats_rgb, feats_opfl, feat_mask, templates, collect_states=False,
                                                            trim=False)
        B, S, L = tag_logp.shape
        allow = None
        if word_cat is not None:
            allow = allow_masks(templates if constraints is None else constraints, L, built=built and constraints is not None)
            allow = allow.to(pos_feats.device)
        seq, seq_logp, score, key = cap_model.beam_captions_ruled(feats_rgb, feats_opfl, feat_mask, pos_feats.reshape(B, S, -1),
                                                                  word_cat=word_cat, allow=allow, **rules)
    return seq, seq_logp, score, key, tag_logp.sum(2)


def score_captions_with_templates(pos_model, cap_model, feats_rgb, feats_opfl, feat_mask, templates, captions, cross=False):
    """Score GIVEN captions of each of the B videos under its S POS templates, on one captioner encoder pass: (tok_logp, score,
    count, template_score (B,S)).  The forced POS rollout (``pos_model.sample_forced``) leaves `pos_feats` (B*S,R) on the device and
    ``cap_model.score_captions_per_video`` (include/xgate_score.h; `captions` (B,N,L'), `cross` and the three results as there:
    (B,S,..) for caption s under template s, (B,S,N,..) with cross=True for every caption under every template) takes the B videos
    once; nothing is read back between the two or after them.  `templates` as in ``caption_with_templates``.  Inference only: both
    models run under ``torch.no_grad()``."""
    with torch.no_grad():
        tag_logp, _, _, pos_feats = pos_model.sample_forced(feats_rgb, feats_opfl, feat_mask, templates, collect_states=False,
                                                            trim=False)
        B, S = tag_logp.shape[:2]
        tok_logp, score, count = cap_model.score_captions_per_video(feats_rgb, feats_opfl, feat_mask, pos_feats.reshape(B, S, -1),
                                                                    captions, cross=cross)
    return tok_logp, score, count, tag_logp.sum(2)


def template_recovery(score):
    """(B,S) bool for a cross score (B,S,S) -- ``score[b, s, n]``: caption n under template s, as ``score_captions_per_video(...,
    cross=True)`` returns it for the S captions generated under the S templates: True where caption s is most likely under ITS OWN
    template s, i.e. no other template gives it a higher score (a tie with another template still counts as recovered).  Torch ops
    on the tensor's device; nothing is read back."""
    t = torch.as_tensor(score)
    if t.dim() != 3 or t.shape[1] != t.shape[2]:
        raise ValueError("score (B,S,S) expected, got %s" % (tuple(t.shape),))
    own = torch.diagonal(t, dim1=1, dim2=2)                                  # (B,S): caption s under template s
    return own >= t.max(dim=1).values                                        # ... against its best template


def first_occurrences(templates):
    """(B,S) bool for templates (B,S,L): True where no EARLIER template of the same video is identical (slot 0 always is), so
    ``templates[first]`` are a video's distinct templates in the order they were drawn.  Torch ops on the tensor's device; nothing
    is read back."""
    t = torch.as_tensor(templates)
    if t.dim() != 3:
        raise ValueError("templates (B,S,L) expected, got %s" % (tuple(t.shape),))
    S = t.shape[1]
    same = (t.unsqueeze(2) == t.unsqueeze(1)).all(3)                         # (B,S,S): template s equals template s'
    earlier = torch.ones(S, S, dtype=torch.bool, device=t.device).tril(-1)   # [s, s'] : s' < s
    return ~(same & earlier).any(2)


def caption_sampled(pos_model, cap_model, feats_rgb, feats_opfl, feat_mask, S, temperature=1.0, uniforms=None, generator=None,
                    opt={}, share_encoder=False):
    """Caption each of the B videos under S POS templates the generator draws itself: (seq (B,S,n) int64, seqLogprobs (B,S,n),
    templates (B,S,L) int64, template_score (B,S), first (B,S) bool).  The sampled POS rollout (``pos_model.sample_templates``:
    `temperature`, `uniforms`, `generator` as there) leaves `pos_feats` (B*S,R) on the device and the captioner's ``sample``
    (``opt`` as there) runs over the B*S rows exactly as in ``caption_with_templates``; nothing is read back between the two.
    template_score is the untempered log-probability the POS generator gives the drawn template (end tag included); `first`
    marks each video's distinct templates (``first_occurrences``).  Inference only: both models run under ``torch.no_grad()``.
    `share_encoder` as in ``caption_with_templates``."""
    if share_encoder and opt.get("beam_size", 1) > 1:
        raise NotImplementedError("share_encoder=True has no beam search: beam_size must be 1 (beam_captions_with_templates "
                                  "is the beam search on one encoder pass)")
    with torch.no_grad():
        templates, tag_logp, _, _, pos_feats = pos_model.sample_templates(feats_rgb, feats_opfl, feat_mask, S, temperature=temperature,
                                                                          uniforms=uniforms, generator=generator,
                                                                          collect_states=False, trim=False)
        B, S = tag_logp.shape[:2]
        seq, slp = _caption_rows(cap_model, feats_rgb, feats_opfl, feat_mask, pos_feats, B, S, opt, share_encoder)
        first = first_occurrences(templates)
    return seq, slp, templates, tag_logp.sum(2), first


def caption_beam(pos_model, cap_model, feats_rgb, feats_opfl, feat_mask, beam_size=5, suppress_tag=1, opt={}, share_encoder=False):
    """Caption each of the B videos under the W = beam_size POS templates the generator itself finds most likely: (seq (B,W,n)
    int64, seqLogprobs (B,W,n), templates (B,W,L) int64, score (B,W)), a video's templates best first.  The beam search
    (``pos_model.beam_templates``: `beam_size`, `suppress_tag` as there) runs without a host synchronisation and its templates go
    through ``caption_with_templates``.  `pos_feats` come from that forced replay: the search permutes its slots at every step and
    overwrites dead ones, so it ends with no held state per returned beam to hand over.  `score` is the beam's summed
    log-probability at its finish (with the -1000 of a suppressed tag, should the beam hold one), not the replay's template score.
    Inference only: both models run under ``torch.no_grad()``.  `share_encoder` as in ``caption_with_templates`` (it is the
    CAPTIONER's beam search, opt["beam_size"] > 1, that it does not serve; `beam_size` here is the POS generator's)."""
    if share_encoder and opt.get("beam_size", 1) > 1:
        raise NotImplementedError("share_encoder=True has no beam search: beam_size must be 1 (beam_captions_with_templates "
                                  "is the beam search on one encoder pass)")
    with torch.no_grad():
        templates, _, score, _ = pos_model.beam_templates(feats_rgb, feats_opfl, feat_mask, beam_size=beam_size,
                                                          suppress_tag=suppress_tag, trim=False)
        seq, slp, _ = caption_with_templates(pos_model, cap_model, feats_rgb, feats_opfl, feat_mask, templates, opt,
                                             share_encoder=share_encoder)
    return seq, slp, templates, score


def caption_beam_diverse(pos_model, cap_model, feats_rgb, feats_opfl, feat_mask, groups, group_size, diversity=0.5, suppress_tag=1,
                         opt={}, share_encoder=False):
    """``caption_beam`` over the DIVERSE POS search: caption each of the B videos under the N = groups * group_size templates of
    ``pos_model.beam_templates_diverse`` (`groups`, `group_size`, `diversity`, `suppress_tag` as there; include/
    xgate_pos_beam_diverse.h): (seq (B,N,n) int64, seqLogprobs (B,N,n), templates (B,N,L) int64, score (B,N), first (B,N) bool).
    Template g * group_size + k is the k-th best of group g; `score` is its penalised sum at the finish; `first` marks each
    video's distinct templates (``first_occurrences``).  The search runs without a host synchronisation and its templates go
    through ``caption_with_templates`` (`opt`, `share_encoder` as in ``caption_beam``).  Inference only: both models run under
    ``torch.no_grad()``."""
    if share_encoder and opt.get("beam_size", 1) > 1:
        raise NotImplementedError("share_encoder=True has no beam search: beam_size must be 1 (beam_captions_with_templates "
                                  "is the beam search on one encoder pass)")
    with torch.no_grad():
        templates, _, score, _ = pos_model.beam_templates_diverse(feats_rgb, feats_opfl, feat_mask, groups, group_size,
                                                                  diversity=diversity, suppress_tag=suppress_tag, trim=False)
        templates, score = templates.flatten(1, 2), score.flatten(1, 2)
        seq, slp, _ = caption_with_templates(pos_model, cap_model, feats_rgb, feats_opfl, feat_mask, templates, opt,
                                             share_encoder=share_encoder)
        first = first_occurrences(templates)
    return seq, slp, templates, score, first
