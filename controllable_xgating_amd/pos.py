"""The POS sequence generator (reference pos_src/SAModel.py): the model whose greedy rollout states become the captioner's global
POS feature (pos_src/eval_utils.py:36-75 writes them, caption_src/data_io.py:215-217 reads the last row).

fp32 products.  ``PosModel`` keeps the reference's class surface and state_dict (43 entries: a reference checkpoint loads with
``strict=True``); its eval forward and greedy ``sample`` run the HIP entry points of include/xgate_pos.h, one host synchronisation per
call (the reference's data-dependent lengths T' and n are computed on the device).  In train mode the teacher-forced forward runs
include/xgate_pos_train.h (BatchNorm over the batch statistics, hash dropout) and ``loss.backward()`` its HIP backward; the parameters
live in one flat buffer (``flat_parameters()`` / ``flat_grads()``) so that ``train.ClipAdam`` updates them in one launch.  Train-mode
``sample()``, ``sample(beam_size > 1)`` and ``sample(sample_max=0)`` are not implemented and raise.  ``sample_forced`` rolls the
generator along a caller's POS templates, several per video (include/xgate_pos_control.h), ``sample_templates`` draws the templates
from the generator's own distribution, several per video (include/xgate_pos_sample.h), and ``beam_templates`` returns the W
templates the generator itself finds most likely for each video (beam search on the device, include/xgate_pos_beam.h); control.py
carries each of these results into the captioner.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _native as nv
from . import _native_pos as npos
from . import _native_pos_train as npt
from ._plumbing import FlatParams, _Holder, _stream, bn_struct, bump_bn, next_seed


class PosModel(FlatParams, nn.Module):
    """reference pos_src/SAModel.py:13-184 (eval-mode inference)."""

    def __init__(self, opt):
        super().__init__()
        self.category_size = opt.category_size
        self.input_encoding_size = opt.input_encoding_size
        self.rnn_size = opt.rnn_size
        self.att_size = opt.att_size
        self.num_layers = getattr(opt, "num_layers", 1)
        self.drop_prob_lm = opt.drop_prob_lm
        self.seq_length = opt.seq_length
        self.feat_size, self.feat_size2 = opt.feat_size, opt.feat_size2
        R, E, A, Cn = self.rnn_size, self.input_encoding_size, self.att_size, self.category_size
        enc = _Holder()
        enc.visual_emb_rgb = nn.Sequential(nn.Linear(opt.feat_size, R), nn.BatchNorm1d(R), nn.ReLU(True))
        enc.visual_emb_opfl = nn.Sequential(nn.Linear(opt.feat_size2, R), nn.BatchNorm1d(R), nn.ReLU(True))
        enc.lstmcell_rgb = nn.LSTMCell(R, R)
        enc.lstmcell_opfl = nn.LSTMCell(R, R)
        enc.fusion = _Holder()
        enc.fusion.late_fusion = nn.Sequential(nn.Linear(2 * R, R), nn.ReLU(), nn.Dropout(self.drop_prob_lm))
        self.two_fc_encoder = enc
        self.img_embed_h_1 = nn.Linear(R, R)
        self.img_embed_c_1 = nn.Linear(R, R)
        core = _Holder()
        core.lstmcell = _Holder()
        core.lstmcell.i2h = nn.Linear(E, 4 * R)
        core.lstmcell.a2h = nn.Linear(R, 4 * R)
        core.lstmcell.h2h = nn.Linear(R, 4 * R)
        core.v2a = nn.Linear(R, A)
        core.h2a = nn.Linear(R, A)
        core.a2w = nn.Linear(A, 1)
        self.lstmcore = core
        self.embed = nn.Embedding(Cn, E)
        self.logit = nn.Linear(R, Cn)
        with torch.no_grad():                       # SAModel.py:37-42
            self.embed.weight.uniform_(-0.1, 0.1)
            self.logit.bias.fill_(0)
            self.logit.weight.uniform_(-0.1, 0.1)
        self._ws = {}
        self._cws = None                # workspace of sample_forced / sample_templates / beam_templates (grows to the largest call)
        self._tws = None                # training workspace: the saved activations of the last train-mode forward
        self._train_gen = 0             # bumped by every train-mode forward: a backward of an older one must not read them
        self._call = 0
        self.dropout_seed = None        # fixed seed of the dropout hash (tests: a checker regenerates the masks); None = fresh per call
        self.ss_prob = 0.0              # accepted and ignored: both branches of SAModel.py:76-79 feed the ground truth

    # ---- native plumbing
    def _check_eval(self, *tensors):
        if self.training:
            raise NotImplementedError("this PosModel entry point runs in eval mode only (call .eval()): train mode covers the "
                                      "teacher-forced forward and its backward")
        self._check_device(*tensors)

    def _check_device(self, *tensors):
        for t in tensors:
            if not t.is_cuda:
                raise nv.XgError("PosModel needs CUDA (HIP) tensors: there is no CPU / PyTorch fallback")
        for p in self.parameters():
            if not p.is_cuda or p.dtype != torch.float32:
                raise nv.XgError("PosModel parameters must be fp32 on the GPU (model.cuda())")

    def _abi(self):
        npos.lib()
        return npos.PARAM_NAMES, npos.XgpParams

    def _refuse_host_params(self, first):
        if not first.is_cuda:
            raise nv.XgError("PosModel trains on the GPU only: call model.cuda() first (no CPU path)")

    def mark_params_changed(self, **kw):
        """train.ClipAdam's notice that a kernel rewrote the flat buffer.  Nothing to do: every call reads the parameters afresh
        (the decoder's packed tiles are rebuilt per call)."""

    def _run(self):
        r = npt.XgptRun()
        r.train = 1 if self.training else 0
        r.drop_p = float(self.drop_prob_lm or 0.0)
        r.seed = next_seed(self)
        r.bn_momentum = 0.1
        return r

    def _bump_bn(self, n=1):
        bump_bn(self.two_fc_encoder, self.training, n)

    def _train_workspace(self, dims, device):
        n = npt.lib().xgpt_workspace_bytes(C.byref(dims))
        if n == 0:
            raise nv.XgError("xgpt_workspace_bytes: invalid dims")
        if self._tws is None or self._tws.device != device or self._tws.numel() < n:
            self._tws = torch.empty(n, dtype=torch.uint8, device=device)
        return self._tws

    def _params(self):
        plist = self._plist()
        for n, p in zip(npos.PARAM_NAMES, plist):
            if not p.is_contiguous():
                raise nv.XgError("parameter %s is not contiguous" % n)
        return npos.XgpParams(*[p.data_ptr() for p in plist])

    def _bn(self):
        return bn_struct(self.two_fc_encoder)

    def _dims(self, B, K, T):
        return npos.XgpDims(B, K, self.rnn_size, self.att_size, self.input_encoding_size, self.category_size, self.feat_size,
                            self.feat_size2, T)

    def _workspace(self, dims, device):
        L = npos.lib()
        n = L.xgp_workspace_bytes(C.byref(dims))
        if n == 0:
            raise nv.XgError("xgp_workspace_bytes: invalid dims")
        key = (device.index, n)
        ws = self._ws.get(key)
        if ws is None:
            self._ws.clear()
            ws = torch.zeros(n, dtype=torch.uint8, device=device)
            self._ws[key] = ws
        return ws

    @staticmethod
    def _feats(feats_rgb, feats_opfl, feat_mask):
        f = [t.float().contiguous() for t in (feats_rgb, feats_opfl, feat_mask)]
        if f[0].dim() != 3 or f[1].shape[:2] != f[0].shape[:2] or tuple(f[2].shape) != tuple(f[0].shape[:2]):
            raise nv.XgError("feats_rgb (B,K,F1), feats_opfl (B,K,F2), feat_mask (B,K) expected")
        return f

    def _rows_feats(self, feats_rgb, feats_opfl, feat_mask):
        """The opening of the rows calls (sample_forced / sample_templates / beam_templates): (fr, fo, fm, B, K)."""
        self._check_eval(feats_rgb, feats_opfl, feat_mask)
        fr, fo, fm = self._feats(feats_rgb, feats_opfl, feat_mask)
        return (fr, fo, fm) + tuple(fm.shape)

    def _rows_setup(self, workspace_bytes, B, K, rows, dev, invalid):
        """What every rows call passes to the library: (dims for seq_length + 1 steps, params, bn, the shared workspace grown to
        `workspace_bytes(dims, rows)`, n_out).  `invalid`: the error text when the library refuses the dims."""
        dims = self._dims(B, K, self.seq_length + 1)
        nbytes = workspace_bytes(C.byref(dims), rows)
        if nbytes == 0:
            raise nv.XgError(invalid)
        if self._cws is None or self._cws.device != dev or self._cws.numel() < nbytes:
            self._cws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return dims, self._params(), self._bn(), self._cws, torch.empty(1, dtype=torch.int32, device=dev)

    @staticmethod
    def _rows_trim(trim, n_out, by_tag, by_step):
        """`by_tag` (B,S,L) cut to n and `by_step` (B,S,L+1,...) to n + 1 (None stays None) when `trim`: the reference's n, one
        host synchronisation."""
        if not trim:
            return by_tag, by_step
        n = int(n_out.item())                       # the one host synchronisation of the call
        return [t[:, :, :n] for t in by_tag], [None if t is None else t[:, :, :n + 1] for t in by_step]

    # ---- the reference's surface
    def init_hidden(self, feat, feat_mask):
        """SAModel.py:54-60: the encoder output summed over ALL K rows, over the mask count, through img_embed_{h,c}_1 (detached).
        ((1,B,R), (1,B,R)); the native forward / sample compute the same thing on the device."""
        with torch.no_grad():
            mean = (feat.float().sum(1) / feat_mask.float().sum(1, keepdim=True)).unsqueeze(0)
            return self.img_embed_h_1(mean), self.img_embed_c_1(mean)

    def encode(self, feats_rgb, feats_opfl, feat_mask):
        """two_fc_encoder (sub_modules.py:199-239): V (B,K,R)."""
        self._check_eval(feats_rgb, feats_opfl, feat_mask)
        fr, fo, fm = self._feats(feats_rgb, feats_opfl, feat_mask)
        B, K = fm.shape
        dims = self._dims(B, K, 1)
        ws = self._workspace(dims, fr.device)
        V = torch.empty(B, K, self.rnn_size, device=fr.device)
        P, bn = self._params(), self._bn()
        nv.check(npos.lib().xgp_encoder_fwd(_stream(), C.byref(dims), C.byref(P), C.byref(bn), fr.data_ptr(), fo.data_ptr(),
                                            fm.data_ptr(), V.data_ptr(), ws.data_ptr(), ws.numel()), "xgp_encoder_fwd")
        return V

    def forward(self, feats_rgb, feats_opfl, feat_mask, seq, seq_mask, cap_classes, new_mask, return_pos_feats=False):
        """SAModel.py:62-90: teacher-forced log-probabilities (B, T', C) over the already rolled `cap_classes` / `new_mask`
        (prepare_pos_targets); the loop stops at the first i >= 1 whose category column is all zero.  `seq` / `seq_mask` are
        unused, as in the reference.  In train mode: BatchNorm over the batch (running statistics and num_batches_tracked
        updated), dropout, and a result that carries a gradient.

        `return_pos_feats` (train mode only; joint training, docs/JOINT_TRAINING.md): returns (logp, pos_feats), pos_feats (B,R)
        the state behind step T' - 1 -- the vector the captioner consumes (caption_src/data_io.py:215-216) -- with a graph of
        its own: a gradient sent into it reaches the generator's parameters through the same HIP backward.  Under dropout it is
        the state after the step's mask, as the loop carries it.  In eval mode `sample_forced` yields the vector."""
        if return_pos_feats and not self.training:
            raise NotImplementedError("return_pos_feats is the train-mode forward's output: in eval mode sample_forced returns "
                                      "pos_feats for the same tags")
        if self.training:
            for t in (feats_rgb, feats_opfl, feat_mask, cap_classes, new_mask):
                if not t.is_cuda:
                    raise NotImplementedError("PosModel trains on the GPU only: there is no CPU path (model.cuda() and CUDA inputs)")
            self._check_device()
            self._ensure_flat()
            fr, fo, fm = self._feats(feats_rgb, feats_opfl, feat_mask)
            cap = cap_classes.detach().long().contiguous()
            nm = new_mask.detach().float().contiguous()
            if cap.shape[0] != fm.shape[0] or tuple(nm.shape) != tuple(cap.shape):
                raise nv.XgError("cap_classes / new_mask (B,T) expected")
            return _PosTrainFunction.apply(self, bool(return_pos_feats), fr.detach(), fo.detach(), fm.detach(), cap, nm, *self._plist())
        self._check_eval(feats_rgb, feats_opfl, feat_mask, cap_classes, new_mask)
        fr, fo, fm = self._feats(feats_rgb, feats_opfl, feat_mask)
        cap = cap_classes.long().contiguous()
        nm = new_mask.float().contiguous()
        B, K = fm.shape
        T = cap.shape[1]
        if cap.shape[0] != B or tuple(nm.shape) != tuple(cap.shape):
            raise nv.XgError("cap_classes / new_mask (B,T) expected")
        dims = self._dims(B, K, T)
        ws = self._workspace(dims, fr.device)
        logp = torch.empty(B, T, self.category_size, device=fr.device)
        t_out = torch.empty(1, dtype=torch.int32, device=fr.device)
        P, bn = self._params(), self._bn()
        nv.check(npos.lib().xgp_forward_tf(_stream(), C.byref(dims), C.byref(P), C.byref(bn), fr.data_ptr(), fo.data_ptr(),
                                           fm.data_ptr(), cap.data_ptr(), nm.data_ptr(), logp.data_ptr(), t_out.data_ptr(),
                                           ws.data_ptr(), ws.numel()), "xgp_forward_tf")
        Tp = int(t_out.item())                      # the one host synchronisation of the call
        return logp if Tp == T else logp[:, :Tp].contiguous()

    def sample(self, feats_rgb, feats_opfl, feat_mask, opt={}):
        """SAModel.py:136-184, greedy: (seq (B,n), seqLogprobs (B,n), collect_states (B,n+1,R), collect_masks (B,n+1)).  All
        seq_length + 1 steps run on the device (finished rows hold their state exactly), then the outputs are trimmed to the
        reference's n."""
        if opt.get("beam_size", 1) > 1:
            raise NotImplementedError("sample() is the greedy rollout only: POS beam search is beam_templates (the reference's "
                                      "extraction runs --beam_size 1: its sample_beam returns 2 values where eval_utils.py unpacks 4)")
        if not opt.get("sample_max", 1):
            raise NotImplementedError("sampled POS rollouts (sample_max = 0) are not implemented (nor are they in the reference)")
        self._check_eval(feats_rgb, feats_opfl, feat_mask)
        fr, fo, fm = self._feats(feats_rgb, feats_opfl, feat_mask)
        B, K = fm.shape
        T = self.seq_length + 1
        dims = self._dims(B, K, T)
        ws = self._workspace(dims, fr.device)
        dev = fr.device
        seq = torch.empty(B, T - 1, dtype=torch.int64, device=dev)
        slp = torch.empty(B, T - 1, device=dev)
        states = torch.empty(B, T, self.rnn_size, device=dev)
        masks = torch.empty(B, T, device=dev)
        n_out = torch.empty(1, dtype=torch.int32, device=dev)
        P, bn = self._params(), self._bn()
        nv.check(npos.lib().xgp_sample_greedy(_stream(), C.byref(dims), C.byref(P), C.byref(bn), fr.data_ptr(), fo.data_ptr(),
                                              fm.data_ptr(), seq.data_ptr(), slp.data_ptr(), states.data_ptr(), masks.data_ptr(),
                                              n_out.data_ptr(), ws.data_ptr(), ws.numel()), "xgp_sample_greedy")
        n = int(n_out.item())                       # the one host synchronisation of the rollout
        return seq[:, :n], slp[:, :n], states[:, :n + 1], masks[:, :n + 1]

    def sample_forced(self, feats_rgb, feats_opfl, feat_mask, templates, collect_states=True, trim=True):
        """The rollout of `sample` with the greedy choice replaced by the caller's POS templates (include/xgate_pos_control.h),
        S templates for each of the B videos: (tag_logp (B,S,n), states (B,S,n+1,R) or None, masks (B,S,n+1), pos_feats (B*S,R)).

        `templates`: what control.pad_templates takes -- (B,S,L') or (B,L') (one template per video) integer tags with
        L' <= seq_length, or nested lists; entry t-1 is the tag fed at step t, a 0 ends the template and whatever follows it is
        ignored.  tag_logp[b,s,t-1] is the log-probability of tag t given the tags before it, up to and including the end tag, 0
        after it: its sum over the last axis is the template's score.  pos_feats, row b S + s, is the state after the last step:
        the captioner's global POS vector for video b under template s.  `trim`: cut to the reference's n (the longest template,
        one host synchronisation); trim=False returns the full seq_length and does not synchronise.  `collect_states=False`
        skips storing the states."""
        from . import _native_pos_control as npc
        from .control import pad_templates
        fr, fo, fm, B, K = self._rows_feats(feats_rgb, feats_opfl, feat_mask)
        L = self.seq_length
        dev = fr.device
        tm = pad_templates(templates, L, self.category_size).to(dev)
        if tm.shape[0] != B:
            raise ValueError("templates for %d videos, features for %d" % (tm.shape[0], B))
        S = tm.shape[1]
        lib = npc.lib()
        dims, P, bn, ws, n_out = self._rows_setup(lib.xgpc_workspace_bytes, B, K, S, dev,
                                                  "xgpc_workspace_bytes: invalid dims or too many rows (B %d, S %d)" % (B, S))
        tag_logp = torch.empty(B, S, L, device=dev)
        states = torch.empty(B, S, L + 1, self.rnn_size, device=dev) if collect_states else None
        masks = torch.empty(B, S, L + 1, device=dev)
        pos_feats = torch.empty(B * S, self.rnn_size, device=dev)
        nv.check(lib.xgpc_sample_forced(_stream(), C.byref(dims), S, C.byref(P), C.byref(bn), fr.data_ptr(), fo.data_ptr(),
                                        fm.data_ptr(), tm.data_ptr(), tag_logp.data_ptr(),
                                        None if states is None else states.data_ptr(), masks.data_ptr(), pos_feats.data_ptr(),
                                        n_out.data_ptr(), ws.data_ptr(), ws.numel()), "xgpc_sample_forced")
        (tag_logp,), (states, masks) = self._rows_trim(trim, n_out, (tag_logp,), (states, masks))
        return tag_logp, states, masks, pos_feats

    def sample_templates(self, feats_rgb, feats_opfl, feat_mask, S, temperature=1.0, uniforms=None, generator=None,
                         collect_states=False, trim=True):
        """S sampled rollouts for each of the B videos (include/xgate_pos_sample.h): the rollout of `sample` with the greedy
        choice replaced by an inverse-CDF draw over exp(logit / temperature), the captioner's rule.  Returns (templates (B,S,n)
        int64, tag_logp (B,S,n), states (B,S,n+1,R) or None, masks (B,S,n+1), pos_feats (B*S,R)).

        `templates` is zero from a row's first 0 onwards, so it is directly a valid input of `sample_forced`; tag_logp is the
        UNTEMPERED log-probability of each drawn tag up to and including the end tag, 0 after it, and its row sum is the
        template's score, as in the forced call.  `uniforms`: float32 (B,S,L), L = seq_length, one per draw (moved to the device);
        None: ``torch.rand(B,S,L, device=..., generator=generator)``.  No random number generator lives in the library.
        `trim`: cut to the reference's n (one host synchronisation); trim=False returns the full seq_length and does not
        synchronise."""
        from . import _native_pos_sample as nps
        fr, fo, fm, B, K = self._rows_feats(feats_rgb, feats_opfl, feat_mask)
        L = self.seq_length
        dev = fr.device
        S = int(S)
        temperature = float(temperature)
        if S < 1:
            raise ValueError("S >= 1 rollouts per video expected, got %d" % S)
        if not (0.0 < temperature < float("inf")):
            raise ValueError("temperature must be finite and > 0, got %r" % temperature)
        if uniforms is None:
            u = torch.rand(B, S, L, device=dev, generator=generator)
        else:
            u = torch.as_tensor(uniforms)
            if u.dtype != torch.float32 or tuple(u.shape) != (B, S, L):
                raise ValueError("uniforms: float32 (%d,%d,%d) expected, got %s %s" % (B, S, L, u.dtype, tuple(u.shape)))
            u = u.to(dev).contiguous()
        lib = nps.lib()
        dims, P, bn, ws, n_out = self._rows_setup(lib.xgps_workspace_bytes, B, K, S, dev,
                                                  "xgps_workspace_bytes: invalid dims or too many rows (B %d, S %d)" % (B, S))
        templates = torch.empty(B, S, L, dtype=torch.int64, device=dev)
        tag_logp = torch.empty(B, S, L, device=dev)
        states = torch.empty(B, S, L + 1, self.rnn_size, device=dev) if collect_states else None
        masks = torch.empty(B, S, L + 1, device=dev)
        pos_feats = torch.empty(B * S, self.rnn_size, device=dev)
        nv.check(lib.xgps_sample_templates(_stream(), C.byref(dims), S, temperature, C.byref(P), C.byref(bn), fr.data_ptr(),
                                           fo.data_ptr(), fm.data_ptr(), u.data_ptr(), templates.data_ptr(), tag_logp.data_ptr(),
                                           None if states is None else states.data_ptr(), masks.data_ptr(), pos_feats.data_ptr(),
                                           n_out.data_ptr(), ws.data_ptr(), ws.numel()), "xgps_sample_templates")
        (templates, tag_logp), (states, masks) = self._rows_trim(trim, n_out, (templates, tag_logp), (states, masks))
        return templates, tag_logp, states, masks, pos_feats

    def beam_templates(self, feats_rgb, feats_opfl, feat_mask, beam_size=5, suppress_tag=1, trim=True, return_trace=False):
        """The W = beam_size templates the generator itself finds most likely for each of the B videos (include/xgate_pos_beam.h:
        the reference's sample_beam, pos_src/SAModel.py:104-134, run on the device with no host work per step).  Returns (templates
        (B,W,n) int64, tag_logp (B,W,n), score (B,W), masks (B,W,n+1)[, trace (B,L,W,2) int32]).

        A video's beams come best first, each ranked by its summed log-probability `score` at the moment it finished.  `templates`
        is zero after a beam's finish, so it is directly a valid input of `sample_forced`; tag_logp holds the log-probability of
        every tag up to and including the end tag.  `suppress_tag`: the category whose log-probability is lowered by 1000 before
        every merge (the reference does this for category 1); -1 turns it off.  `trim`: cut to the reference's n (one host
        synchronisation); trim=False returns the full seq_length and does not synchronise.  `return_trace`: also the (token, parent
        slot) of every slot and step.  beam_size may not exceed category_size or 8."""
        from . import _native_pos_beam as npb
        fr, fo, fm, B, K = self._rows_feats(feats_rgb, feats_opfl, feat_mask)
        L = self.seq_length
        dev = fr.device
        W, sup = int(beam_size), int(suppress_tag)
        if W < 1 or W > self.category_size or W > npb.XGPB_MAX_BEAM:
            raise ValueError("1 <= beam_size <= min(category_size = %d, %d) expected, got %d" % (self.category_size, npb.XGPB_MAX_BEAM, W))
        if sup >= self.category_size:
            raise ValueError("suppress_tag must lie below category_size = %d (-1: none), got %d" % (self.category_size, sup))
        lib = npb.lib()
        dims, P, bn, ws, n_out = self._rows_setup(lib.xgpb_workspace_bytes, B, K, W, dev,
                                                  "xgpb_workspace_bytes: invalid dims, too many rows (B %d, W %d) or W * rnn_size beyond "
                                                  "the merge kernel's LDS" % (B, W))
        templates = torch.empty(B, W, L, dtype=torch.int64, device=dev)
        tag_logp = torch.empty(B, W, L, device=dev)
        score = torch.empty(B, W, device=dev)
        masks = torch.empty(B, W, L + 1, device=dev)
        trace = torch.empty(B, L, W, 2, dtype=torch.int32, device=dev) if return_trace else None
        nv.check(lib.xgpb_beam_templates(_stream(), C.byref(dims), W, sup, C.byref(P), C.byref(bn), fr.data_ptr(), fo.data_ptr(),
                                         fm.data_ptr(), templates.data_ptr(), tag_logp.data_ptr(), score.data_ptr(), masks.data_ptr(),
                                         n_out.data_ptr(), None if trace is None else trace.data_ptr(), ws.data_ptr(), ws.numel()),
                 "xgpb_beam_templates")
        (templates, tag_logp), (masks,) = self._rows_trim(trim, n_out, (templates, tag_logp), (masks,))
        out = (templates, tag_logp, score, masks)
        return out + (trace,) if return_trace else out

    def beam_templates_diverse(self, feats_rgb, feats_opfl, feat_mask, groups, group_size, diversity=0.5, suppress_tag=1, trim=True,
                               return_trace=False):
        """Diverse beam search (include/xgate_pos_beam_diverse.h): Gd = groups beam searches of width Wg = group_size per video, a
        group steered away from the tags the groups before it took at the same step by `diversity` (lambda >= 0) per live slot that
        took them.  Returns (templates (B,Gd,Wg,n) int64, tag_logp (B,Gd,Wg,n), score (B,Gd,Wg), masks (B,Gd,Wg,n+1)[, trace
        (B,L,N,2) int32]), N = Gd Wg <= min(category_size, 8).

        A group's beams come best first, ranked by the PENALISED sum `score` at the moment they finished; tag_logp holds the
        unpenalised log-probabilities.  `templates.flatten(1, 2)` is a valid input of `sample_forced`.  groups = 1 is
        `beam_templates(beam_size=group_size)` bit for bit.  suppress_tag, trim and return_trace as in `beam_templates`; the
        trace's parents are slot indices of the video."""
        from . import _native_pos_beam_diverse as npd
        if self.training:
            self._check_eval()                          # (raises: eval mode only)
        Gd, Wg, sup, lam = int(groups), int(group_size), int(suppress_tag), float(diversity)
        most = min(self.category_size, npd.XGPD_MAX_BEAM)
        # (the search's own checks hold on any device: behind the mode's gate, ahead of the device's, as in the captioner's search)
        if Gd < 1 or Wg < 1 or Gd * Wg > most:
            raise ValueError("groups, group_size >= 1 and groups * group_size <= min(category_size = %d, %d) expected, got %d, %d"
                             % (self.category_size, npd.XGPD_MAX_BEAM, Gd, Wg))
        if not (0.0 <= lam < float("inf")):
            raise ValueError("diversity must be finite and >= 0, got %r" % (diversity,))
        if sup >= self.category_size:
            raise ValueError("suppress_tag must lie below category_size = %d (-1: none), got %d" % (self.category_size, sup))
        fr, fo, fm, B, K = self._rows_feats(feats_rgb, feats_opfl, feat_mask)
        L = self.seq_length
        dev = fr.device
        lib = npd.lib()
        N = Gd * Wg
        dims, P, bn, ws, n_out = self._rows_setup(lambda d, n: lib.xgpd_workspace_bytes(d, Gd, Wg), B, K, N, dev,
                                                  "xgpd_workspace_bytes: invalid dims, too many rows (B %d, N %d) or N * rnn_size beyond "
                                                  "the merge kernel's LDS" % (B, N))
        templates = torch.empty(B, Gd, Wg, L, dtype=torch.int64, device=dev)
        tag_logp = torch.empty(B, Gd, Wg, L, device=dev)
        score = torch.empty(B, Gd, Wg, device=dev)
        masks = torch.empty(B, Gd, Wg, L + 1, device=dev)
        trace = torch.empty(B, L, N, 2, dtype=torch.int32, device=dev) if return_trace else None
        nv.check(lib.xgpd_beam_templates(_stream(), C.byref(dims), Gd, Wg, lam, sup, C.byref(P), C.byref(bn), fr.data_ptr(),
                                         fo.data_ptr(), fm.data_ptr(), templates.data_ptr(), tag_logp.data_ptr(), score.data_ptr(),
                                         masks.data_ptr(), n_out.data_ptr(), None if trace is None else trace.data_ptr(), ws.data_ptr(),
                                         ws.numel()), "xgpd_beam_templates")
        if trim:
            n = int(n_out.item())                       # the one host synchronisation of the call
            templates, tag_logp, masks = templates[..., :n], tag_logp[..., :n], masks[..., :n + 1]
        out = (templates, tag_logp, score, masks)
        return out + (trace,) if return_trace else out

class _PosTrainFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, want_pos, fr, fo, fm, cap, nm, *params):
        B, K = fm.shape
        T = cap.shape[1]
        dev = fr.device
        dims = model._dims(B, K, T)
        ws = model._train_workspace(dims, dev)
        logp = torch.empty(B, T, model.category_size, device=dev)
        t_out = torch.empty(1, dtype=torch.int32, device=dev)
        run = model._run()
        P, bn = model._params(), model._bn()
        nv.check(npt.lib().xgpt_forward_train(_stream(), C.byref(dims), C.byref(P), C.byref(bn), C.byref(run), fr.data_ptr(),
                                              fo.data_ptr(), fm.data_ptr(), cap.data_ptr(), nm.data_ptr(), logp.data_ptr(),
                                              t_out.data_ptr(), ws.data_ptr(), ws.numel()), "xgpt_forward_train")
        model._bump_bn()
        model._train_gen += 1
        Tp = int(t_out.item())                      # the one host synchronisation of the iteration
        ctx.model, ctx.dims, ctx.run, ctx.Tp, ctx.gen, ctx.keep = model, dims, run, Tp, model._train_gen, (fr, fo, fm)
        out = logp if Tp == T else logp[:, :Tp].contiguous()
        if not want_pos:
            return out
        from . import _native_pos_joint as npj
        pos = torch.empty(B, model.rnn_size, device=dev)
        nv.check(npj.lib().xgpj_final_state(_stream(), C.byref(dims), Tp, ws.data_ptr(), ws.numel(), pos.data_ptr()),
                 "xgpj_final_state")
        ctx.set_materialize_grads(False)            # an output nobody differentiates sends None, not a zero tensor
        return out, pos

    @staticmethod
    def backward(ctx, dlogp, dpos=None):
        model = ctx.model
        if model._train_gen != ctx.gen or model._tws is None:
            raise nv.XgError("PosModel backward: a later train-mode forward has overwritten this forward's saved activations "
                             "(call backward before the next forward)")
        fr, fo, fm = ctx.keep
        ws = model._tws
        g, gs = model._grads_struct()
        run = ctx.run
        if dlogp is None and dpos is None:
            return (None,) * (7 + len(npos.PARAM_NAMES))
        dl = None if dlogp is None else dlogp.detach().float().contiguous()
        if dpos is None:
            nv.check(npt.lib().xgpt_backward(_stream(), C.byref(ctx.dims), C.byref(model._params()), C.byref(gs), C.byref(run),
                                             fr.data_ptr(), fo.data_ptr(), fm.data_ptr(), ctx.Tp, dl.data_ptr(), ws.data_ptr(),
                                             ws.numel()), "xgpt_backward")
        else:
            from . import _native_pos_joint as npj
            dp = dpos.detach().float().contiguous()
            nv.check(npj.lib().xgpj_backward(_stream(), C.byref(ctx.dims), C.byref(model._params()), C.byref(gs), C.byref(run),
                                             fr.data_ptr(), fo.data_ptr(), fm.data_ptr(), ctx.Tp, None if dl is None else dl.data_ptr(),
                                             ws.data_ptr(), ws.numel(), dp.data_ptr()), "xgpj_backward")
        return (None,) * 7 + tuple(model._grad_views(g))


class ClassiferCriterion(nn.Module):
    """pos_src/SAModel.py:201-218: masked NLL with the target rolled LEFT by one and an optional class mask (unlike the
    captioner's criterion of the same name).  A forward that stopped early (T' < T) is scored on the first T' columns of the rolled
    target and masks.  The loss carries a gradient when its input requires one."""

    def forward(self, input, target, mask, class_mask=None):
        if not input.is_cuda:
            raise nv.XgError("ClassiferCriterion needs CUDA (HIP) tensors")
        B, Tp, Cn = input.shape
        target = target.long()
        if Tp == target.shape[1]:
            tgt, roll = target.contiguous(), 1
        else:
            tgt, roll = torch.cat([target[:, 1:], target[:, :1]], 1)[:, :Tp].contiguous(), 0
        m = mask[:, :Tp].float().contiguous()
        m2 = None if class_mask is None else class_mask[:, :Tp].float().contiguous()
        if input.requires_grad and torch.is_grad_enabled():
            from .model import _NLLFunction
            return _NLLFunction.apply(input, tgt, m, m2, roll)
        logp = input.detach().float().contiguous()
        out = torch.empty(2, device=input.device)
        nv.check(nv.lib().xg_nll_fwd(_stream(), logp.data_ptr(), tgt.data_ptr(), m.data_ptr(),
                                     None if m2 is None else m2.data_ptr(), B, Tp, Cn, roll, out.data_ptr()), "xg_nll_fwd")
        return out[0] / out[1]


def prepare_pos_targets(cap_classes, class_mask, check=True):
    """starttrain_trainpos.py:132-136 / eval_utils.py:46-50: the categories rolled RIGHT by one (the last column becomes the BOS
    column) and new_mask = 1 up to and including the last non-zero of each row's class_mask.  `check`: raise when a row of
    class_mask has no non-zero entry (a host synchronisation for a device tensor); unchecked, such a row gets new_mask all ones."""
    cap_classes = torch.as_tensor(cap_classes)
    class_mask = torch.as_tensor(class_mask)
    rolled = torch.cat([cap_classes[:, -1:], cap_classes[:, :-1]], dim=-1)
    T = class_mask.shape[1]
    nz = class_mask != 0
    if check and not bool(nz.any(1).all()):
        raise ValueError("every row of class_mask needs a non-zero entry (the reference indexes its last one)")
    last = (T - 1) - torch.flip(nz, dims=[1]).int().argmax(1)
    new_mask = (torch.arange(T, device=class_mask.device).unsqueeze(0) <= last.unsqueeze(1)).to(class_mask.dtype)
    return rolled, new_mask


def extract_pos_features(model, batches, writer, opt=None):
    """pos_src/eval_utils.py:36-75: for every batch (feats_rgb, feats_opfl, feat_mask, cap_classes, class_mask, video_ids) -- the
    raw, un-rolled categories as the collate_fn yields them -- the validation loss of the teacher-forced forward and the greedy
    rollout, whose states go to `writer` (any mapping, e.g. an h5py.File): writer[vid]['states'] (n+1, R), ['masks'] (1, n+1),
    ['tokens'] (1, n).  The first occurrence of a video id wins.  Returns the mean loss over the batches."""
    opt = dict({"sample_max": 1, "beam_size": 1}, **(opt or {}))
    crit = ClassiferCriterion()
    loss_sum, n_batches = 0.0, 0
    for feats_rgb, feats_opfl, feat_mask, cap_classes, class_mask, vids in batches:
        cap_r, new_mask = prepare_pos_targets(cap_classes, class_mask)
        dev = feats_rgb.device
        cap_r, new_mask, class_mask = cap_r.to(dev), new_mask.to(dev), torch.as_tensor(class_mask).to(dev)
        out = model(feats_rgb, feats_opfl, feat_mask, None, None, cap_r, new_mask)
        # eval_utils.py:51 passes cap_mask as the mask; the captions' mask and new_mask cover the same positions (BOS + words)
        loss_sum += float(crit(out, cap_r, new_mask, class_mask))
        n_batches += 1
        seq, _, states, masks = model.sample(feats_rgb, feats_opfl, feat_mask, opt)
        states, masks, seq = states.cpu().numpy(), masks.cpu().numpy(), seq.cpu().numpy()
        for i, vid in enumerate(vids):
            if vid in writer:
                continue
            grp = {"states": np.ascontiguousarray(states[i]), "masks": masks[i:i + 1].copy(), "tokens": seq[i:i + 1].copy()}
            if hasattr(writer, "create_group"):
                g = writer.create_group(vid)
                for k, v in grp.items():
                    g[k] = v
            else:
                writer[vid] = grp
    return loss_sum / max(n_batches, 1)
