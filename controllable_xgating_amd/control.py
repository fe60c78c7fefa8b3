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
(``SAModel.beam_captions_per_video``, include/xgate_beam_control.h).
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
