"""Host-side mirror of the reference's model surface (caption_src/SAModel.py:13-267) on top of the
HIP C ABI (include/xgate.h).  Same class / method / attribute names, argument meaning, return
shapes and ``state_dict`` keys as the reference, so ``starttrain.py`` / ``eval_utils.py`` style
drivers run unchanged:

    model = SAModel(opt); model.cuda(); model.train()
    logp, cat_logp = model(feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask)
    loss = LanguageModelCriterion()(logp, seq, seq_mask); loss.backward()
    seq, seqLogprobs = model.sample(feats_rgb, feats_opfl, feat_mask, pos_feats, {'sample_max': 0})

PyTorch is plumbing here: tensor allocation, the stream, autograd bookkeeping.  All arithmetic
runs in hand-written gfx950 kernels behind ``libxgate_hip.so``; the nn.Linear / nn.LSTMCell /
nn.BatchNorm1d sub-modules below are parameter CONTAINERS only (they give the reference's
``state_dict`` names, shapes and default initialisation) and are never called.
"""
from __future__ import annotations

import argparse
import ctypes as C

import torch
import torch.nn as nn

from . import _native as nv
from ._plumbing import FlatParams, _Holder, _stream, bn_struct, bump_bn, next_seed  # noqa: F401 (_stream: imported from here by callers)


def make_opt(d=None, **kw):
    """argparse-style namespace with the flags SAModel reads (caption_src/myopts.py:3-88)."""
    base = dict(seed=1024, vocab_size=20000, category_size=14, input_encoding_size=468, rnn_size=512,
                num_layers=1, drop_prob_lm=0.0, seq_length=20, feat_size=1536, feat_size2=1024,
                att_size=1536, fusion_activity="ReLU")
    if d is not None:
        base.update(vocab_size=d.V, category_size=d.C, input_encoding_size=d.E, rnn_size=d.R,
                    seq_length=d.L, feat_size=d.F1, feat_size2=d.F2, att_size=d.A)
    base.update(kw)
    return argparse.Namespace(**base)


def _with_grad_event(model, run):
    """XgRun for ONE backward call: carries the "decoder-side gradients are final" event (XgRun.grad_event) when a
    data-parallel helper (train.GradSync) has armed one on the model; otherwise the forward's XgRun as it is."""
    ev = getattr(model, "_grad_event", None)
    if ev is None:
        return run
    r = nv.XgRun()
    C.memmove(C.byref(r), C.byref(run), C.sizeof(nv.XgRun))
    r.grad_event = ev.cuda_event
    ev_head = getattr(model, "_grad_event_head", None)
    if ev_head is not None:
        r.grad_event_head = ev_head.cuda_event
    return r


# side-stream handles of the library (xg_aux_create: two HIP streams + events each), ONE per (device, caller stream) for the
# whole process and never destroyed: every model on that stream shares it.  A handle per model would add two more HIP streams
# per model, and streams beyond the first handful share the hardware's compute pipes with the earlier ones -- see
# train.shared_stream for what that costs.
_AUX_HANDLES = {}


class _WorkspacePool:
    """Caller-owned workspaces (xg_workspace_bytes).  A forward that saves activations for a
    backward keeps its workspace until the backward has run; everything else shares scratch."""

    def __init__(self, gemm_mode=0):
        self.free = {}
        self.scratch = {}
        self.gemm_mode = gemm_mode            # sizes the workspaces: only the bf16 mode carries the bf16 mirror region (+50 %)

    @staticmethod
    def _key(dims, device):
        return (tuple(getattr(dims, f[0]) for f in dims._fields_), str(device))

    def _alloc(self, dims, device):
        n = nv.lib().xg_workspace_bytes_mode(C.byref(dims), self.gemm_mode)
        if n == 0:
            raise nv.XgError("xg_workspace_bytes_mode: invalid dims")
        return torch.zeros(n + 256, dtype=torch.uint8, device=device)     # zero-filled at first use: include/xgate.h

    def take(self, dims, device):
        lst = self.free.setdefault(self._key(dims, device), [])
        return lst.pop() if lst else self._alloc(dims, device)

    def give(self, dims, device, ws):
        self.free.setdefault(self._key(dims, device), []).append(ws)

    def shared(self, dims, device):
        k = self._key(dims, device)
        if k not in self.scratch:
            self.scratch[k] = self._alloc(dims, device)
        return self.scratch[k]


def _ws_ptr(ws):
    p = ws.data_ptr()
    p = (p + 255) & ~255
    return C.c_void_p(p), C.c_size_t(ws.numel() - 256)


class SAModel(FlatParams, nn.Module):
    """Drop-in for reference caption_src/SAModel.py:SAModel (CaptionModel(nn.Module))."""

    def __init__(self, opt):
        super().__init__()
        nv.lib()  # fail loudly, right here, if the HIP library is missing
        seed = opt.seed
        torch.manual_seed(seed)
        self.vocab_size = opt.vocab_size
        self.category_size = opt.category_size
        self.input_encoding_size = opt.input_encoding_size
        self.rnn_size = opt.rnn_size
        self.visual_size = opt.rnn_size
        self.num_layers = opt.num_layers
        self.drop_prob_lm = opt.drop_prob_lm
        self.seq_length = opt.seq_length
        self.att_size = opt.att_size
        self.feat_size, self.feat_size2 = opt.feat_size, opt.feat_size2
        self.ss_prob = 0.0
        self.done_beams = []
        R, E, A, p = opt.rnn_size, opt.input_encoding_size, opt.att_size, opt.drop_prob_lm

        def gate(src, tgt):  # reference sub_modules.py:18-31 (re-seeds, so siblings start identical)
            torch.manual_seed(seed)
            h = _Holder()
            h.gate = nn.Sequential(nn.Linear(src, tgt), nn.ReLU(), nn.Dropout(p))
            return h

        # construction order mirrors the reference so torch's default init consumes the RNG identically
        enc = _Holder()
        torch.manual_seed(seed)                                                    # sub_modules.py:86
        enc.visual_emb_rgb = nn.Sequential(nn.Linear(opt.feat_size, R), nn.BatchNorm1d(R), nn.ReLU(True))
        enc.visual_emb_opfl = nn.Sequential(nn.Linear(opt.feat_size2, R), nn.BatchNorm1d(R), nn.ReLU(True))
        enc.drop_out = nn.Dropout(p)
        enc.lstmcell_rgb = nn.LSTMCell(R, R)
        enc.lstmcell_opfl = nn.LSTMCell(R, R)
        enc.gate_rgb = gate(R, R)
        enc.gate_opfl = gate(R, R)
        torch.manual_seed(seed)                                                    # Fusion, sub_modules.py:55
        enc.fusion = _Holder()
        enc.fusion.late_fusion = nn.Sequential(nn.Linear(2 * R, R), getattr(nn, opt.fusion_activity)(), nn.Dropout(p))
        self.two_spatial_encoder = enc
        self.img_embed_h_1 = nn.Linear(R, R)
        self.img_embed_c_1 = nn.Linear(R, R)
        self.img_embed_h_2 = nn.Linear(R, R)
        self.img_embed_c_2 = nn.Linear(R, R)
        core = _Holder()
        torch.manual_seed(seed)                                                    # sub_modules.py:648
        core.gate = gate(E, R)

        def cell(in1):
            c = _Holder()
            c.i2h, c.a2h, c.h2h = nn.Linear(in1, 4 * R), nn.Linear(R, 4 * R), nn.Linear(R, 4 * R)
            c.dropout = nn.Dropout(p)
            return c

        core.lstm_1 = cell(E)
        core.lstm_2 = cell(R)
        core.dropout = nn.Dropout(p)
        core.v2a = nn.Linear(R, A)
        core.h2a = nn.Linear(2 * R, A)
        core.a2w = nn.Linear(A, 1)
        self.lstmcore = core
        self.embed = nn.Embedding(self.vocab_size, E)
        self.logit = nn.Linear(R, self.vocab_size)
        self.classifer = nn.Sequential(nn.Linear(R, 128), nn.ReLU(), nn.Dropout(p), nn.Linear(128, self.category_size))
        self.init_weights()
        if getattr(opt, "fusion_activity", "ReLU") != "ReLU":
            raise ValueError("only fusion_activity='ReLU' (the shipped recipe) is implemented in HIP")
        self._pool = _WorkspacePool({"fp32": 0, "bf16": 1, "bf16x3": 3}.get(getattr(opt, "precision", "fp32"), 1))
        self._call = 0
        self.dropout_seed = None        # fixed seed of the dropout hash (tests / bench parity leg: a checker can regenerate the same masks); None = a fresh seed per call
        self._packed = None          # recurrent weights in MFMA-fragment order (xg_pack_weights), refreshed lazily
        self._packed_key = None
        self._packed_epoch = 0
        # arithmetic of the large GEMMs: 'fp32' (exact fp32 MFMA), 'bf16x3' (split-bf16, fp32-class accuracy, faster),
        # 'bf16' (bf16 operands / fp32 accumulate, for the large AND the per-step products: BASELINE.json configs[4]).
        # 'bf16x3' splits the per-step products too (three bf16 planes of the packed fp32 tiles, xg_step.hip PREC 2).
        self.precision = getattr(opt, "precision", "fp32")
        if self.precision not in ("fp32", "bf16", "bf16x3"):
            raise ValueError("precision must be 'fp32', 'bf16x3' or 'bf16'")

    def init_weights(self):  # SAModel.py:52-56
        initrange = 0.1
        self.embed.weight.data.uniform_(-initrange, initrange)
        self.logit.bias.data.fill_(0)
        self.logit.weight.data.uniform_(-initrange, initrange)

    # ------------------------------------------------------------------ plumbing
    def _abi(self):
        return nv.PARAM_NAMES, nv.XgParams

    def _param_list(self):
        return self._plist()

    def _bn_struct(self):
        return bn_struct(self.two_spatial_encoder)

    def _dims(self, B, K, T):
        d = nv.XgDims()
        d.B, d.K, d.R, d.A, d.E, d.V = B, K, self.rnn_size, self.att_size, self.input_encoding_size, self.vocab_size
        d.C, d.H, d.F1, d.F2, d.T = self.category_size, 128, self.feat_size, self.feat_size2, T
        return d

    def mark_params_changed(self, only_encoder_since_pack_early=False):
        """Tell the model its parameters were rewritten behind torch's back (a HIP kernel on the flat buffer, e.g.
        train.ClipAdam.step): the packed shadow of the recurrent weights is rebuilt before the next call.  Updates made
        through torch on the parameters themselves (optimizers, load_state_dict, ``p.copy_()``, ``p.mul_()`` under
        no_grad) are noticed by themselves (tensor version counters).  NOT noticed: in-place writes through ``p.data``
        (``p.data.copy_()``, ``p.data.uniform_()`` -- common in code written against the reference's torch 0.3): ``.data``
        has its own version counter.  Call this method after such writes.
        ``only_encoder_since_pack_early=True`` is the statement of an optimizer that called ``pack_early()`` right behind its
        update of every parameter group except the CG encoder's and has written NOTHING but the encoder's segment of the flat
        buffer since (train.ClipAdam): only then may the next call keep the early-packed decoder tiles.  Any other caller gets
        the full re-pack."""
        self._packed_epoch += 1
        if not only_encoder_since_pack_early:
            self._early_key = None           # whatever pack_early() covered may be stale again: the next call re-packs everything

    def _packed_dtype(self):
        """Element type of the packed recurrent weights (include/xgate.h: XgRun.packed_dtype): bf16 tiles for the bf16 arithmetic,
        three pre-split bf16 planes for split-bf16, fp32 tiles otherwise."""
        over = getattr(self, "_packed_dtype_override", None)      # tests: split-bf16 over plain fp32 tiles (split in registers)
        return {"bf16": 1, "bf16x3": 2}.get(self.precision, 0) if over is None else over

    def pack_early(self):
        """For an optimizer that has JUST updated every parameter group except the CG encoder's on the current stream (and will
        call mark_params_changed() when the rest is done): refresh the packed tiles of the decoder's matrices here and now, under
        the encoder's backward, instead of at the head of the next iteration (xg_pack_weights_part, part 1).  The next
        _packed_ptr() then only packs the encoder's tiles (and, with bf16 tiles, the bf16 copies of the encoder's weights).  No-op
        when there is nothing to gain (no shadow yet, a HIP-graph capture)."""
        if self._packed is None or torch.cuda.is_current_stream_capturing():
            return
        self._ensure_flat()
        dtype = self._packed_dtype()
        key = (self._flat.data_ptr(), self._flat._version, self._packed_epoch, dtype, tuple(p._version for p in self._plist()))
        d = self._dims(1, 1, 1)
        nbytes = nv.lib().xg_packed_bytes(C.byref(d), dtype)
        if nbytes == 0 or self._packed.numel() < nbytes + 16:
            return
        ptr = (self._packed.data_ptr() + 15) & ~15
        ps = self._params_struct()
        nv.check(nv.lib().xg_pack_weights_part(_stream(), C.byref(d), C.byref(ps), C.c_void_p(ptr), C.c_size_t(nbytes), dtype, 1, 1),
                 "xg_pack_weights_part")
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        # valid for exactly the NEXT epoch (the optimizer's mark_params_changed) with nothing else changed in between
        self._early_event, self._early_epoch, self._early_key = ev, self._packed_epoch + 1, key[:2] + key[3:]

    def _aux_handle(self):
        """Side-stream handle (include/xgate.h: xg_aux_create) for the current device and stream, created on first use."""
        if torch.cuda.is_current_stream_capturing():
            return None      # a HIP graph is being captured: one stream (forked streams crash or replay slowly, train.GraphedXEStep)
        st = torch.cuda.current_stream()
        key = (st.device.index, st.cuda_stream)
        h = _AUX_HANDLES.get(key)
        if h is None:
            out = C.c_void_p()
            nv.check(nv.lib().xg_aux_create(C.byref(out)), "xg_aux_create")
            h = _AUX_HANDLES[key] = out.value
        return h

    def _packed_ptr(self):
        """Device pointer of the packed recurrent weights (include/xgate.h: xg_pack_weights), valid for the current
        parameter values; None when the shapes do not allow it (rnn_size % 8 != 0)."""
        self._ensure_flat()
        dtype = self._packed_dtype()
        key = (self._flat.data_ptr(), self._flat._version, self._packed_epoch, dtype,
               tuple(p._version for p in self._plist()))
        if key != self._packed_key:
            d = self._dims(1, 1, 1)
            nbytes = nv.lib().xg_packed_bytes(C.byref(d), dtype)
            if nbytes == 0:
                self._packed = None
            else:
                fresh = self._packed is None or self._packed.device != self._flat.device or self._packed.numel() < nbytes + 16
                if fresh:
                    self._packed = torch.empty(nbytes + 16, dtype=torch.uint8, device=self._flat.device)
                ptr = (self._packed.data_ptr() + 15) & ~15
                ps = self._params_struct()
                # the decoder's matrices may already have been refreshed behind the optimizer's update of their parameter group
                # (pack_early, under the CG encoder's backward): then only the encoder's four tiles are left for the head of the
                # iteration, behind an event that completed long ago
                early = (not fresh and getattr(self, "_early_key", None) == key[:2] + key[3:] and
                         self._early_epoch == self._packed_epoch and not torch.cuda.is_current_stream_capturing())
                if early:
                    torch.cuda.current_stream().wait_event(self._early_event)
                    nv.check(nv.lib().xg_pack_weights_part(_stream(), C.byref(d), C.byref(ps), C.c_void_p(ptr), C.c_size_t(nbytes), dtype, 1, 2),
                             "xg_pack_weights_part")
                else:
                    nv.check(nv.lib().xg_pack_weights(_stream(), C.byref(d), C.byref(ps), C.c_void_p(ptr), C.c_size_t(nbytes), dtype, 1),
                             "xg_pack_weights")
                self._early_key = None
                # the shadow is (re)written on THIS stream: calls on any other stream must wait for it (a rollout on a side
                # stream right after an optimizer step, driver.scst_rollouts(mode="streams"))
                if torch.cuda.is_current_stream_capturing():       # (a HIP graph: ordering is the graph's own business)
                    self._packed_event = None
                else:
                    st = torch.cuda.current_stream()
                    ev = torch.cuda.Event()
                    ev.record(st)
                    self._packed_event, self._packed_stream = ev, (st.device.index, st.cuda_stream)
            self._packed_key = key
        if self._packed is None:
            return None
        ev = getattr(self, "_packed_event", None)
        if ev is not None:
            st = torch.cuda.current_stream()
            if (st.device.index, st.cuda_stream) != self._packed_stream:
                st.wait_event(ev)
        return (self._packed.data_ptr() + 15) & ~15

    def _run(self, save, seed=None):
        r = nv.XgRun()
        r.train = 1 if self.training else 0
        r.drop_p = float(self.drop_prob_lm)
        r.seed = next_seed(self, seed)
        r.save = 1 if save else 0
        r.bn_momentum, r.bn_eps = 0.1, 1e-5
        r.gemm_mode = {"fp32": 0, "bf16": 1, "bf16x3": 3}[self.precision]
        r.packed = self._packed_ptr()
        r.packed_dtype = self._packed_dtype()
        r.aux = self._aux_handle()
        pe = getattr(self, "_prof_events", None)       # measurement hook (bench.py): a pair of timing events around the T decoder steps
        if pe is not None:
            r.prof_event0, r.prof_event1 = pe[0].cuda_event, pe[1].cuda_event
        return r

    @staticmethod
    def _batch(feats_rgb, feats_opfl, feat_mask, pos_feats, seq=None, seq_mask=None):
        def f32(t):
            return t.detach().contiguous().float()
        keep = [f32(feats_rgb), f32(feats_opfl), f32(feat_mask), f32(pos_feats),
                None if seq is None else seq.detach().contiguous().long(),
                None if seq_mask is None else f32(seq_mask)]
        for t in keep:
            if t is not None and not t.is_cuda:
                raise nv.XgError("inputs must be CUDA (HIP) tensors")
        b = nv.XgBatch()
        b.feats_rgb, b.feats_opfl, b.feat_mask, b.pos_feats = (t.data_ptr() for t in keep[:4])
        b.seq = keep[4].data_ptr() if keep[4] is not None else None
        b.seq_mask = keep[5].data_ptr() if keep[5] is not None else None
        return b, keep

    def _bump_bn(self, n=1):
        bump_bn(self.two_spatial_encoder, self.training, n)

    # ------------------------------------------------------------------ reference surface
    def forward(self, feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask):
        """SAModel.forward (SAModel.py:67-115): (m,K,F) x2, (m,K), (m,R), (m,T) int64, (m,T) ->
        log-probs (m,T,V) and category log-probs (m,T,C).  With self.ss_prob > 0 in train mode the scheduled-sampling
        path (SAModel.py:89-99, xg_forward_ss) runs instead of the hoisted teacher-forced one."""
        params = self._param_list()
        save = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        if self.training and self.ss_prob > 0.0:                                 # scheduled sampling, SAModel.py:89-99
            T, B = seq.shape[1], seq.shape[0]
            u = getattr(self, "ss_uniforms", None)                               # test hook: (u_sel, u_tok), each (T,B)
            if u is None:
                u = (torch.rand(T, B, device=seq.device), torch.rand(T, B, device=seq.device))
            ss = (float(self.ss_prob), u[0].contiguous().float(), u[1].contiguous().float())
            return _XEFunction.apply(self, save, ss, feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, *params)
        return _XEFunction.apply(self, save, None, feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, *params)

    def xe_loss(self, feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes=None,
                class_mask=None, weight_class=0.0):
        """Fused fast path: forward + LanguageModelCriterion (+ weight_class * ClassiferCriterion)
        without materialising the (m,T,V) log-prob tensor or its gradient
        (starttrain.py:125-129).  Returns the scalar loss tensor; .backward() works.

        It teacher-forces whatever ``ss_prob`` is: scheduled sampling on the fused path is ``xe_loss_ss``."""
        params = self._param_list()
        save = _wants_dpos(self, pos_feats, "xe_loss") or (torch.is_grad_enabled() and any(p.requires_grad for p in params))
        return _XELossFunction.apply(self, save, feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes,
                                     class_mask, float(weight_class), *params)

    def _ss_uniforms(self, T, M, dev):
        """(u_sel, u_tok), each (T, M) float32 on `dev`: the test hook ``self.ss_uniforms`` or two fresh draws."""
        u = getattr(self, "ss_uniforms", None)
        if u is None:
            u = (torch.rand(T, M, device=dev), torch.rand(T, M, device=dev))
        u = tuple(t.detach().to(dev).contiguous().float() for t in u)
        for t in u:
            if tuple(t.shape) != (T, M):
                raise ValueError("ss_uniforms: two (%d, %d) tensors expected, got %s" % (T, M, tuple(t.shape)))
        return u

    def xe_loss_ss(self, feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes=None, class_mask=None,
                   weight_class=0.0):
        """``xe_loss`` under scheduled sampling (include/xgate_ss.h; SAModel.py:89-99): in train mode with ``ss_prob`` > 0, row m of
        step t >= 1 is fed a token drawn from step t - 1's distribution iff u_sel[t, m] < ss_prob, else seq[m, t]; the loss is
        ``xe_loss``'s over the logits that token stream produces and no gradient flows through the choice.  The draw happens
        inside the decoder loop on the device: no (m,T,V) log-prob tensor and no gradient of one.  The uniforms come from the test
        hook ``self.ss_uniforms = (u_sel, u_tok)``, each (T, m), else from two ``torch.rand``.  Returns the scalar loss with a
        graph, sets ``last_losses`` and leaves the fed tokens in ``last_ss_tokens`` (T, m) int64.

        Eval mode or ``ss_prob`` == 0: this is ``xe_loss`` (``last_ss_tokens`` is then seq, time-major).  fp32, device tensors."""
        if not (self.training and self.ss_prob > 0.0):
            loss = self.xe_loss(feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes, class_mask, weight_class)
            self.last_ss_tokens = seq.detach().long().t().contiguous()
            return loss
        if self.precision != "fp32":
            raise NotImplementedError("xe_loss_ss is fp32 only (precision = %r)" % (self.precision,))
        for name, t, nd in (("feats_rgb", feats_rgb, 3), ("feats_opfl", feats_opfl, 3), ("feat_mask", feat_mask, 2),
                            ("pos_feats", pos_feats, 2), ("seq", seq, 2), ("seq_mask", seq_mask, 2)):
            if not torch.is_tensor(t) or t.dim() != nd:
                raise ValueError("%s: a %d-dimensional tensor expected" % (name, nd))
        for t in (feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes, class_mask):
            if t is not None and not t.is_cuda:
                raise NotImplementedError("xe_loss_ss needs device tensors: there is no CPU path")
        if not 0.0 <= float(self.ss_prob) <= 1.0:
            raise ValueError("ss_prob in [0, 1] expected, got %r" % (self.ss_prob,))
        params = self._param_list()
        save = _wants_dpos(self, pos_feats, "xe_loss_ss") or (torch.is_grad_enabled() and any(p.requires_grad for p in params))
        u = self._ss_uniforms(int(seq.shape[1]), int(seq.shape[0]), seq.device)
        return _XELossSSFunction.apply(self, save, 0, float(self.ss_prob), u, feats_rgb, feats_opfl, feat_mask, pos_feats, seq,
                                       seq_mask, cap_classes, class_mask, float(weight_class), *params)

    def xe_loss_ss_per_video(self, feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes=None, class_mask=None,
                             weight_class=0.0):
        """``xe_loss_per_video`` under scheduled sampling (include/xgate_ss.h): the shapes of ``xe_loss_per_video`` -- the B videos
        once, pos_feats (B,Q,R), seq / seq_mask (B,Q,T) --, the rule of ``xe_loss_ss`` on the M = B Q rows, row b Q + q.  The
        uniforms of the test hook ``self.ss_uniforms`` are (T, M) each; ``last_ss_tokens`` is (T, M) int64.

        Eval mode or ``ss_prob`` == 0: this is ``xe_loss_per_video``.  fp32, device tensors."""
        if not (self.training and self.ss_prob > 0.0):
            loss = self.xe_loss_per_video(feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes, class_mask,
                                          weight_class)
            self.last_ss_tokens = seq.detach().long().reshape(-1, seq.shape[-1]).t().contiguous()
            return loss
        if self.precision != "fp32":
            raise NotImplementedError("xe_loss_ss_per_video is fp32 only (precision = %r)" % (self.precision,))
        if not 0.0 <= float(self.ss_prob) <= 1.0:
            raise ValueError("ss_prob in [0, 1] expected, got %r" % (self.ss_prob,))
        for name, t, nd in (("feats_rgb", feats_rgb, 3), ("feats_opfl", feats_opfl, 3), ("feat_mask", feat_mask, 2),
                            ("pos_feats", pos_feats, 3), ("seq", seq, 3), ("seq_mask", seq_mask, 3)):
            if not torch.is_tensor(t) or t.dim() != nd:
                raise ValueError("%s: a %d-dimensional tensor expected" % (name, nd))
        B, K = feats_rgb.shape[:2]
        Q, T = int(seq.shape[1]), int(seq.shape[2])
        if B < 1 or K < 1 or Q < 1 or T < 2:
            raise ValueError("B, K, Q >= 1 and T >= 2 expected, got B %d, K %d, Q %d, T %d" % (B, K, Q, T))
        want = (("feats_rgb", feats_rgb, (B, K, self.feat_size)), ("feats_opfl", feats_opfl, (B, K, self.feat_size2)),
                ("feat_mask", feat_mask, (B, K)), ("pos_feats", pos_feats, (B, Q, self.rnn_size)), ("seq", seq, (B, Q, T)),
                ("seq_mask", seq_mask, (B, Q, T)), ("cap_classes", cap_classes, (B, Q, T)), ("class_mask", class_mask, (B, Q, T)))
        for name, t, shape in want:
            if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != shape):
                raise ValueError("%s %s expected, got %s" % (name, shape, tuple(t.shape) if torch.is_tensor(t) else type(t)))
        if seq.is_floating_point() or (cap_classes is not None and cap_classes.is_floating_point()):
            raise ValueError("seq and cap_classes are integer tensors")
        for t in (feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes, class_mask):
            if t is not None and not t.is_cuda:
                raise NotImplementedError("xe_loss_ss_per_video needs device tensors: there is no CPU path")
        params = self._param_list()
        save = _wants_dpos(self, pos_feats, "xe_loss_ss_per_video") or (torch.is_grad_enabled() and any(p.requires_grad for p in params))
        u = self._ss_uniforms(T, B * Q, seq.device)
        return _XELossSSFunction.apply(self, save, Q, float(self.ss_prob), u, feats_rgb, feats_opfl, feat_mask, pos_feats, seq,
                                       seq_mask, cap_classes, class_mask, float(weight_class), *params)

    def _ss_video_workspace(self, d, Q, dev, save):
        """(key, tensor) of a workspace of xe_loss_ss_per_video (xgss_workspace_bytes): pooled as _video_workspace pools its own."""
        from . import _native_ss as nss
        key = (tuple(getattr(d, f[0]) for f in d._fields_), Q, str(dev))
        pool = self.__dict__.setdefault("_ss_video_pool", {})
        lst = pool.setdefault((key, save), [])
        if lst:
            return key, (lst.pop() if save else lst[0])
        n = nss.lib().xgss_workspace_bytes(C.byref(d), Q)
        if n == 0:
            raise nv.XgError("xgss_workspace_bytes: invalid dims or too many rows (B %d, Q %d)" % (d.B, Q))
        ws = torch.empty(n + 256, dtype=torch.uint8, device=dev)
        if not save:
            lst.append(ws)
        return key, ws

    def xe_loss_per_video(self, feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes=None,
                          class_mask=None, weight_class=0.0):
        """``xe_loss`` for Q captions per video on ONE encoder pass (include/xgate_train_video.h): the B videos are handed over
        once -- feats_rgb (B,K,F1), feats_opfl (B,K,F2), feat_mask (B,K) -- with pos_feats (B,Q,R), seq (B,Q,T) int64, seq_mask
        (B,Q,T) and, optionally, cap_classes (B,Q,T) and class_mask (B,Q,T) per caption; row b Q + q is caption q of video b.
        Returns the scalar loss over the B Q rows with a graph; ``backward()`` fills every parameter gradient and ``last_losses``
        holds (total, language, classifier) as after ``xe_loss``.

        The encoder, init_hidden and v2a(V) run once per video, forward and backward, and every attention step reads a video's V
        and v2a(V) once per group of its rows.  At drop_prob_lm = 0 the loss and the gradients are those of ``xe_loss`` on the
        batch with every video repeated Q times (up to summation order); the BatchNorm running statistics receive the update of
        the B videos.  Under dropout the encoder's masks are those of a B-video call, the decoder's those of a B Q-row call.

        fp32, device tensors, no scheduled sampling (ss_prob = 0); train and eval mode."""
        from . import _native_train_video  # noqa: F401  (the binding is declared when the call is made)
        if self.precision != "fp32":
            raise NotImplementedError("xe_loss_per_video is fp32 only (precision = %r)" % (self.precision,))
        if self.training and self.ss_prob > 0.0:
            raise NotImplementedError("xe_loss_per_video has no scheduled sampling: ss_prob must be 0")
        for name, t, nd in (("feats_rgb", feats_rgb, 3), ("feats_opfl", feats_opfl, 3), ("feat_mask", feat_mask, 2),
                            ("pos_feats", pos_feats, 3), ("seq", seq, 3), ("seq_mask", seq_mask, 3)):
            if not torch.is_tensor(t) or t.dim() != nd:
                raise ValueError("%s: a %d-dimensional tensor expected" % (name, nd))
        B, K = feats_rgb.shape[:2]
        Q, T = int(seq.shape[1]), int(seq.shape[2])
        if B < 1 or K < 1 or Q < 1 or T < 2:
            raise ValueError("B, K, Q >= 1 and T >= 2 expected, got B %d, K %d, Q %d, T %d" % (B, K, Q, T))
        want = (("feats_rgb", feats_rgb, (B, K, self.feat_size)), ("feats_opfl", feats_opfl, (B, K, self.feat_size2)),
                ("feat_mask", feat_mask, (B, K)), ("pos_feats", pos_feats, (B, Q, self.rnn_size)), ("seq", seq, (B, Q, T)),
                ("seq_mask", seq_mask, (B, Q, T)), ("cap_classes", cap_classes, (B, Q, T)), ("class_mask", class_mask, (B, Q, T)))
        for name, t, shape in want:
            if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != shape):
                raise ValueError("%s %s expected, got %s" % (name, shape, tuple(t.shape) if torch.is_tensor(t) else type(t)))
        if seq.is_floating_point() or (cap_classes is not None and cap_classes.is_floating_point()):
            raise ValueError("seq and cap_classes are integer tensors")
        for t in (feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes, class_mask):
            if t is not None and not t.is_cuda:
                raise NotImplementedError("xe_loss_per_video needs device tensors: there is no CPU path")
        params = self._param_list()
        save = _wants_dpos(self, pos_feats, "xe_loss_per_video") or (torch.is_grad_enabled() and any(p.requires_grad for p in params))
        return _XELossVideoFunction.apply(self, save, feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes,
                                          class_mask, float(weight_class), *params)

    def _video_workspace(self, d, Q, dev, save):
        """(key, tensor) of a workspace of xe_loss_per_video (xgtv_workspace_bytes): the forward's own until its backward has run
        when it saves activations, else one shared scratch per shape; not zero-filled (the calls do not read what it held)."""
        from . import _native_train_video as ntv
        key = (tuple(getattr(d, f[0]) for f in d._fields_), Q, str(dev))
        pool = self.__dict__.setdefault("_video_pool", {})
        lst = pool.setdefault((key, save), [])
        if lst:
            return key, (lst.pop() if save else lst[0])
        n = ntv.lib().xgtv_workspace_bytes(C.byref(d), Q)
        if n == 0:
            raise nv.XgError("xgtv_workspace_bytes: invalid dims or too many rows (B %d, Q %d)" % (d.B, Q))
        ws = torch.empty(n + 256, dtype=torch.uint8, device=dev)
        if not save:
            lst.append(ws)
        return key, ws

    def rollout_per_video(self, feats_rgb, feats_opfl, feat_mask, pos_feats, temperature=1.0, uniforms=None, trim=False):
        """The sampled rollout of ``sample`` for S `pos_feats` rows per video on ONE encoder pass, WITH a graph (include/
        xgate_scst_video.h): the B videos are handed over once -- feats_rgb (B,K,F1), feats_opfl (B,K,F2), feat_mask (B,K) -- with
        pos_feats (B,S,R); row b S + s is rollout s of video b.  Returns seq (B,S,L) int64, seqLogprobs (B,S,L) and n (1,) int32 on
        the device (the early-exit width: no host sync); with trim=True the two tensors cut to n (the call's only host sync).
        ``seqLogprobs.backward(...)`` / a criterion on it (PerVideoRewardCriterion) fills every parameter gradient.

        Row by row this is ``sample(..., {'sample_max': 0})`` on the batch with every video repeated S times, uniforms (L + 1, B*S)
        and the untempered log-probability gathered.  The encoder, init_hidden and v2a(V) run once per video, forward and backward;
        the BatchNorm running statistics receive ONE update from the B videos; under dropout the encoder's masks are those of a
        B-video call, the decoder's those of a B S-row call (docs/CAPTION_SCST_PER_VIDEO.md).  Without grad it still runs: train-
        or eval-mode sampling with nothing kept.  fp32 and device tensors only."""
        from . import _native_scst_video  # noqa: F401  (the binding is declared when the call is made)
        if self.precision != "fp32":
            raise NotImplementedError("rollout_per_video is fp32 only (precision = %r)" % (self.precision,))
        for name, t, nd in (("feats_rgb", feats_rgb, 3), ("feats_opfl", feats_opfl, 3), ("feat_mask", feat_mask, 2),
                            ("pos_feats", pos_feats, 3)):
            if not torch.is_tensor(t) or t.dim() != nd:
                raise ValueError("%s: a %d-dimensional tensor expected" % (name, nd))
        B, K = feats_rgb.shape[:2]
        S, L = int(pos_feats.shape[1]), self.seq_length
        if B < 1 or K < 1 or S < 1:
            raise ValueError("B, K, S >= 1 expected, got B %d, K %d, S %d" % (B, K, S))
        for name, t, shape in (("feats_rgb", feats_rgb, (B, K, self.feat_size)), ("feats_opfl", feats_opfl, (B, K, self.feat_size2)),
                               ("feat_mask", feat_mask, (B, K)), ("pos_feats", pos_feats, (B, S, self.rnn_size))):
            if tuple(t.shape) != shape:
                raise ValueError("%s %s expected, got %s" % (name, shape, tuple(t.shape)))
        if not (float(temperature) > 0.0):
            raise ValueError("temperature > 0 expected, got %r" % (temperature,))
        if uniforms is not None and (not torch.is_tensor(uniforms) or tuple(uniforms.shape) != (L + 1, B * S)):
            raise ValueError("uniforms (L + 1 = %d, B*S = %d) expected, got %s"
                             % (L + 1, B * S, tuple(uniforms.shape) if torch.is_tensor(uniforms) else type(uniforms)))
        for t in (feats_rgb, feats_opfl, feat_mask, pos_feats, uniforms):
            if t is not None and not t.is_cuda:
                raise NotImplementedError("rollout_per_video needs device tensors: there is no CPU path")
        params = self._param_list()
        save = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        seq, slp, n = _RolloutVideoFunction.apply(self, save, feats_rgb, feats_opfl, feat_mask, pos_feats, uniforms,
                                                  float(temperature), *params)
        if trim:
            k = int(n.item())
            return seq[:, :, :k], slp[:, :, :k], n
        return seq, slp, n

    def _scst_video_workspace(self, d, S, dev, save):
        """(key, tensor) of a workspace of rollout_per_video (xgsv_workspace_bytes), pooled as _video_workspace pools its own: the
        forward's until its backward has run when it saves activations, else one shared scratch per shape; not zero-filled."""
        from . import _native_scst_video as nsv
        key = (tuple(getattr(d, f[0]) for f in d._fields_), S, str(dev))
        pool = self.__dict__.setdefault("_scst_video_pool", {})
        lst = pool.setdefault((key, save), [])
        if lst:
            return key, (lst.pop() if save else lst[0])
        n = nsv.lib().xgsv_workspace_bytes(C.byref(d), S)
        if n == 0:
            raise nv.XgError("xgsv_workspace_bytes: invalid dims or too many rows (B %d, S %d)" % (d.B, S))
        ws = torch.empty(n + 256, dtype=torch.uint8, device=dev)
        if not save:
            lst.append(ws)
        return key, ws

    def sample_pair(self, feats_rgb, feats_opfl, feat_mask, pos_feats, opt={}):
        """The two rollouts of one SCST iteration in ONE batched pass: ``sample(..., {'sample_max': 0})``
        (starttrain.py:131) and the greedy baseline ``sample(..., {'sample_max': 1})`` (myutils.py:45-48).
        Returns (gen (m,L), sample_logprobs (m,L) [differentiable], greedy (m,L), n (2,) int32 device tensor: the
        reference's early-exit lengths of the two rollouts -- trim with them, or hand n[:1] to RewardCriterion).
        In train mode the BatchNorm running statistics end up exactly where the reference's TWO sample() calls leave
        them (two momentum updates with the unbiased N/(N-1) variance of the un-repeated batch).  With train-mode dropout
        (drop_prob_lm > 0) the two rollouts run as two calls with independent masks, like the reference's -- unless
        self.dropout_seed is set: then both calls take that one seed and so the same masks (a checker regenerates both from it).
        opt["one_pass"] (train-mode dropout only; inert otherwise): the two rollouts still run as ONE 2m-row pass, each half under
        its own seed -- the two seeds the two calls would take, drawn in the same order (docs/SCST_DROPOUT.md).
        opt["return_greedy_logprobs"]: the greedy rollout's (m,L) log-probs as a fifth value."""
        temperature = float(opt.get("temperature", 1.0))
        params = self._param_list()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        want_glp = bool(opt.get("return_greedy_logprobs", False))
        if self.training and self.drop_prob_lm > 0.0 and opt.get("one_pass", False):
            # ... in ONE 2m-row pass all the same (docs/SCST_DROPOUT.md): the library gives rows [m, 2m) the masks of a call of their
            # own under a second seed and runs the encoder once per seed (xgpr_rollout_pair_videos)
            out = _RolloutPairFunction.apply(self, feats_rgb, feats_opfl, feat_mask, pos_feats, opt.get("uniforms", None),
                                             temperature, need_grad, True, *params)
            return out if want_glp else out[:4]
        if self.training and self.drop_prob_lm > 0.0:
            # Train-mode dropout: the reference's two sample() calls (starttrain.py:131, myutils.py:45) draw INDEPENDENT masks,
            # in the encoder and img_embed as well as in the decoder.  The one-batch form below runs the encoder once and would
            # hand both halves the same encoder realisation, so this case takes the reference's own shape: two rollouts, two
            # seeds (each with its BatchNorm update), the greedy one without saved activations.
            uni = opt.get("uniforms", None)
            gen, slp, n_s = _RolloutFunction.apply(self, feats_rgb, feats_opfl, feat_mask, pos_feats, nv.XG_ROLLOUT_SAMPLE, uni,
                                                   None, temperature, need_grad, True, *params)
            with torch.no_grad():
                greedy, glp, n_g = _RolloutFunction.apply(self, feats_rgb, feats_opfl, feat_mask, pos_feats, nv.XG_ROLLOUT_GREEDY,
                                                          None, None, 1.0, False, True, *params)
            out = (gen, slp, greedy, torch.cat([n_s.reshape(1), n_g.reshape(1)]))
            return out + (glp,) if want_glp else out
        out = _RolloutPairFunction.apply(self, feats_rgb, feats_opfl, feat_mask, pos_feats, opt.get("uniforms", None),
                                         temperature, need_grad, False, *params)
        return out if want_glp else out[:4]

    def init_hidden(self, feat, feat_mask):
        """SAModel.init_hidden (SAModel.py:58-65) -> [(h1,c1),(h2,c2)], each (1,m,R)."""
        B, K, R = feat.shape
        d = self._dims(B, K, 1)
        ws = self._pool.shared(d, feat.device)
        wp, wn = _ws_ptr(ws)
        state = torch.empty(4, B, R, dtype=torch.float32, device=feat.device)
        fm = feat_mask.detach().contiguous().float()
        if fm.dim() == 1:
            fm = fm.unsqueeze(0).expand(B, K).contiguous()
        ps = self._params_struct()
        nv.check(nv.lib().xg_init_hidden(_stream(), C.byref(d), C.byref(ps), nv.ptr(feat.detach().contiguous().float()),
                                         nv.ptr(fm), wp, wn, nv.ptr(state)), "xg_init_hidden")
        return [(state[0:1], state[1:2]), (state[2:3], state[3:4])]

    def encode(self, feats_rgb, feats_opfl, feat_mask):
        """two_spatial_encoder(feats_rgb, feats_opfl, feat_mask) (sub_modules.py:118-159), no grad."""
        B, K, _ = feats_rgb.shape
        d = self._dims(B, K, 1)
        ws = self._pool.shared(d, feats_rgb.device)
        wp, wn = _ws_ptr(ws)
        b, keep = self._batch(feats_rgb, feats_opfl, feat_mask, feats_rgb.new_zeros(B, self.rnn_size))
        V = torch.empty(B, K, self.rnn_size, dtype=torch.float32, device=feats_rgb.device)
        ps, bn, run = self._params_struct(), self._bn_struct(), self._run(False)
        nv.check(nv.lib().xg_encoder_fwd(_stream(), C.byref(d), C.byref(ps), C.byref(bn), C.byref(b), C.byref(run),
                                         wp, wn, nv.ptr(V)), "xg_encoder_fwd")
        self._bump_bn()
        return V

    def get_logprobs_state(self, it, feats, pos_feats, state):
        """SAModel.get_logprobs_state (SAModel.py:117-127): one step, mask of ones."""
        B, K, R = feats.shape
        d = self._dims(B, K, 1)
        ws = self._pool.shared(d, feats.device)
        wp, wn = _ws_ptr(ws)
        feats = feats.detach().contiguous().float()
        st = torch.cat([state[0][0], state[0][1], state[1][0], state[1][1]], 0).contiguous().float()
        v2a = self.lstmcore.v2a
        key = (feats.data_ptr(), feats._version, B, K, v2a.weight._version, v2a.bias._version, self._packed_epoch, self.precision)
        if getattr(self, "_vproj_key", None) != key:
            self._vproj_cache = torch.empty(B, K, self.att_size, dtype=torch.float32, device=feats.device)
            ps, run0 = self._params_struct(), self._run(False)
            nv.check(nv.lib().xg_vproj(_stream(), C.byref(d), C.byref(ps), nv.ptr(feats), nv.ptr(self._vproj_cache), C.byref(run0)),
                     "xg_vproj")
            self._vproj_key = key
            self._vproj_feats = feats
        logp = torch.empty(B, self.vocab_size, dtype=torch.float32, device=feats.device)
        ps, run = self._params_struct(), self._run(False)
        pos = pos_feats.detach().contiguous().float()
        tok = it.detach().contiguous().long().to(feats.device)
        nv.check(nv.lib().xg_step_fwd(_stream(), C.byref(d), C.byref(ps), nv.ptr(tok), None, nv.ptr(feats),
                                      nv.ptr(self._vproj_cache), nv.ptr(pos), C.byref(run), 0, wp, wn, nv.ptr(st),
                                      nv.ptr(logp), None), "xg_step_fwd")
        return logp, [(st[0:1], st[1:2]), (st[2:3], st[3:4])]

    def sample(self, feats_rgb, feats_opfl, feat_mask, pos_feats, opt={}):
        """SAModel.sample (SAModel.py:163-219) -> seq (m,n) int64, seqLogprobs (m,n)."""
        sample_max = opt.get("sample_max", 1)
        beam_size = opt.get("beam_size", 1)
        temperature = opt.get("temperature", 1.0)
        if beam_size > 1:
            if opt.get("beam_on_device", False):        # the whole search on the device; done_beams stays as it is
                seq, slp, _ = self.beam_captions(feats_rgb, feats_opfl, feat_mask, pos_feats, beam_size=beam_size,
                                                 suppress_token=opt.get("suppress_token", 1))
                return seq[:, 0], slp[:, 0]
            from .beam import sample_beam
            feats = self.encode(feats_rgb, feats_opfl, feat_mask)
            return sample_beam(self, feats, feat_mask, pos_feats, opt)
        mode = nv.XG_ROLLOUT_GREEDY if sample_max else nv.XG_ROLLOUT_SAMPLE
        forced = opt.get("forced_tokens", None)
        if forced is not None:
            mode = nv.XG_ROLLOUT_REPLAY
        need_grad = torch.is_grad_enabled() and mode != nv.XG_ROLLOUT_GREEDY and any(p.requires_grad for p in self.parameters())
        params = self._param_list()
        uniforms = opt.get("uniforms", None)
        bn_update = bool(opt.get("bn_update", True))
        seq, slp, n = _RolloutFunction.apply(self, feats_rgb, feats_opfl, feat_mask, pos_feats, mode, uniforms, forced,
                                             float(temperature), need_grad, bn_update, *params)
        if opt.get("async", False):            # no host sync: full-width (m, L) tensors + the device-side n
            return seq, slp, n
        n = int(n.item())                      # ONE host sync per rollout (the reference syncs every step, :206)
        return seq[:, :n], slp[:, :n]

    def sample_beam(self, feats, feat_masks, pos_feats, opt={}):
        from .beam import sample_beam
        return sample_beam(self, feats, feat_masks, pos_feats, opt)

    def _search_gate(self, name, *tensors):
        """What the device searches (sample_per_video, beam_captions) require: eval mode, fp32, and `tensors` on the device.
        Called at the head of an entry point without tensors, and with them once its own arguments have been checked."""
        if self.training:
            raise NotImplementedError("%s runs in eval mode only: call model.eval() first" % name)
        if self.precision != "fp32":
            raise NotImplementedError("%s is fp32 only (precision = %r)" % (name, self.precision))
        for t in tensors:
            if not t.is_cuda:
                raise NotImplementedError("%s needs device tensors: there is no CPU path" % name)

    def _search_workspace(self, attr, key, nbytes, dev, invalid):
        """(pointer, bytes) of a device search's workspace, kept in the dict `attr` as {key: tensor} for ONE shape at a time
        (an evaluation runs one batch shape).  `nbytes()`: the library's size for this shape; `invalid`: the error text when
        it refuses the dims."""
        ws = getattr(self, attr, {}).get(key)
        if ws is None:
            n = nbytes()
            if n == 0:
                raise nv.XgError(invalid)
            ws = torch.empty(n + 256, dtype=torch.uint8, device=dev)
            setattr(self, attr, {key: ws})
        return _ws_ptr(ws)

    def _search_open(self, name, inputs, per_video, beam=None, refuse=()):
        """The checks the device searches share, in one order: the gate; `refuse`, the entry point's own (condition, text) pairs;
        the beam arguments `beam` = (W, suppress_token); the (B,S,R) shape of pos_feats (`per_video`); the gate on the tensors
        `inputs` = (feats_rgb, feats_opfl, feat_mask, pos_feats).  Returns (B, K, S or None, L, device, dims at T = L + 1)."""
        from ._native_beam import XGCB_MAX_BEAM
        self._search_gate(name)
        for cond, text in refuse:
            if cond:
                raise NotImplementedError(text)
        if beam is not None:
            W, sup = beam
            if W < 1 or W > self.vocab_size or W > XGCB_MAX_BEAM:
                raise ValueError("1 <= beam_size <= min(vocab_size = %d, %d) expected, got %d" % (self.vocab_size, XGCB_MAX_BEAM, W))
            if sup >= self.vocab_size:
                raise ValueError("suppress_token must lie below vocab_size = %d (-1: none), got %d" % (self.vocab_size, sup))
        (B, K), pos = inputs[0].shape[:2], inputs[3]
        if per_video and (pos.dim() != 3 or pos.shape[0] != B or pos.shape[1] < 1 or pos.shape[2] != self.rnn_size):
            raise ValueError("pos_feats (B = %d, S, R = %d) expected, got %s" % (B, self.rnn_size, tuple(pos.shape)))
        self._search_gate(name, *inputs)
        L = self.seq_length
        return B, K, int(pos.shape[1]) if per_video else None, L, inputs[0].device, self._dims(B, K, L + 1)

    def _search_call(self, attr, key, nbytes, invalid, inputs):
        """What a device search hands the library besides its own arguments and outputs: the cached workspace and the parameter,
        BatchNorm, batch ((B,S,R) pos_feats as its B S rows) and run structs -> (those four by reference in the ABI's order,
        workspace pointer, bytes, what has to outlive the call)."""
        wp, wn = self._search_workspace(attr, key, nbytes, inputs[0].device, invalid)
        with torch.no_grad():
            b, keep = self._batch(*inputs[:3], inputs[3].reshape(-1, self.rnn_size) if inputs[3].dim() == 3 else inputs[3])
            own = (self._params_struct(), self._bn_struct(), b, self._run(False))
        return [C.byref(o) for o in own], wp, wn, (keep, own)

    def sample_per_video(self, feats_rgb, feats_opfl, feat_mask, pos_feats, opt={}):
        """``sample`` for S `pos_feats` rows per video on ONE encoder pass (include/xgate_control.h): the B videos are handed over
        once, `pos_feats` is (B,S,R), and the result is what ``sample`` gives on the batch with every video repeated S times, row by
        row: seq (B,S,n) int64 and seqLogprobs (B,S,n).  The encoder, init_hidden and v2a(V) run once per video and every step's
        attention reads a video's v2a(V) and V once per group of its rows; one enqueue, no host work per step.

        `opt` as in ``sample``: `sample_max` (1: greedy), `temperature`, `uniforms` (L + 1, B*S), `async` (no host sync: full-width
        (B,S,L) tensors and the device-side n).  Eval mode, fp32 and device tensors only; `beam_size` > 1 and `forced_tokens` are not
        served.  Nothing returned carries an autograd graph."""
        from . import _native_control as ncc
        inputs = (feats_rgb, feats_opfl, feat_mask, pos_feats)
        B, K, S, L, dev, d = self._search_open("sample_per_video", inputs, True, refuse=(
            (opt.get("beam_size", 1) > 1, "sample_per_video has no beam search: beam_size must be 1"),
            (opt.get("forced_tokens", None) is not None, "sample_per_video has no replay mode: forced_tokens must be None")))
        M = B * S
        mode = nv.XG_ROLLOUT_GREEDY if opt.get("sample_max", 1) else nv.XG_ROLLOUT_SAMPLE
        temperature = float(opt.get("temperature", 1.0))
        uniforms = opt.get("uniforms", None)
        if mode == nv.XG_ROLLOUT_SAMPLE:
            if uniforms is None:
                uniforms = torch.rand(L + 1, M, device=dev, dtype=torch.float32)
            uniforms = uniforms.detach().contiguous().float()
            if tuple(uniforms.shape) != (L + 1, M) or not uniforms.is_cuda:
                raise ValueError("uniforms (L + 1 = %d, B*S = %d) on the device expected, got %s" % (L + 1, M, tuple(uniforms.shape)))
        else:
            uniforms = None
        lib = ncc.lib()
        args, wp, wn, keep = self._search_call("_control_ws", (B, K, L, S, str(dev)), lambda: lib.xgcc_workspace_bytes(C.byref(d), S),
                                               "xgcc_workspace_bytes: invalid dims or too many rows (B %d, S %d)" % (B, S), inputs)
        seq = torch.empty(B, S, L, dtype=torch.int64, device=dev)
        slp = torch.empty(B, S, L, dtype=torch.float32, device=dev)
        n = torch.empty(1, dtype=torch.int32, device=dev)
        nv.check(lib.xgcc_rollout(_stream(), C.byref(d), S, *args, mode, nv.ptr(uniforms), temperature, nv.ptr(seq), nv.ptr(slp),
                                  nv.ptr(n), wp, wn), "xgcc_rollout")
        if opt.get("async", False):
            return seq, slp, n
        n = int(n.item())
        return seq[:, :, :n], slp[:, :, :n]

    def sample_truncated_per_video(self, feats_rgb, feats_opfl, feat_mask, pos_feats, top_k=0, top_p=1.0, temperature=1.0,
                                   uniforms=None, generator=None, return_stats=False, trim=True):
        """``sample_per_video`` in sampled mode with TOP-K and NUCLEUS truncation (include/xgate_truncate.h, docs/CAPTION_TRUNCATED.md):
        every word is drawn from softmax(logits / temperature) restricted to the `top_k` largest logits (0: off) and, inside those,
        to the smallest set of whole value classes whose mass reaches `top_p` (1: off); ties at either threshold are kept.
        `pos_feats` is (B,S,R) -- (B,1,R) is the plain one-row-per-video case.  Returns (seq (B,S,n) int64, seqLogprobs (B,S,n)):
        the log-probabilities are the UNTEMPERED, UNTRUNCATED ones, as ``sample`` gives them.  ``return_stats=True`` adds seq_logq
        (B,S,n), the log-probability under the distribution actually drawn from (what an importance weight or a reranker needs),
        and kept (B,S,n) int32, the size of the kept set; both are 0 behind a row's end token.

        `uniforms` (L + 1, B*S) on the device; None: ``torch.rand(L + 1, B*S, device=..., generator=generator)``.  ``trim=False``:
        no host sync -- full-width (B,S,L) tensors and the device-side n after them.  Eval mode, fp32 and device tensors only;
        one enqueue, no host work per step.  Nothing returned carries an autograd graph."""
        from . import _native_truncate as ntr
        self._search_gate("sample_truncated_per_video")
        top_k, top_p, temperature = int(top_k), float(top_p), float(temperature)
        if top_k < 0:
            raise ValueError("top_k >= 0 expected (0: off), got %d" % top_k)
        if not (0.0 < top_p <= 1.0):
            raise ValueError("top_p in (0, 1] expected (1: off), got %r" % top_p)
        if not (0.0 < temperature < float("inf")):
            raise ValueError("temperature must be finite and > 0, got %r" % temperature)
        inputs = (feats_rgb, feats_opfl, feat_mask, pos_feats)
        B, K, S, L, dev, d = self._search_open("sample_truncated_per_video", inputs, True)
        M = B * S
        if uniforms is None:
            uniforms = torch.rand(L + 1, M, device=dev, dtype=torch.float32, generator=generator)
        uniforms = uniforms.detach().contiguous().float()
        if tuple(uniforms.shape) != (L + 1, M) or not uniforms.is_cuda:
            raise ValueError("uniforms (L + 1 = %d, B*S = %d) on the device expected, got %s" % (L + 1, M, tuple(uniforms.shape)))
        lib = ntr.lib()
        args, wp, wn, keep = self._search_call("_control_ws", (B, K, L, S, str(dev)), lambda: lib.xgtr_workspace_bytes(C.byref(d), S),
                                               "xgtr_workspace_bytes: invalid dims or too many rows (B %d, S %d)" % (B, S), inputs)
        seq = torch.empty(B, S, L, dtype=torch.int64, device=dev)
        slp = torch.empty(B, S, L, dtype=torch.float32, device=dev)
        slq = torch.empty(B, S, L, dtype=torch.float32, device=dev) if return_stats else None
        kept = torch.empty(B, S, L, dtype=torch.int32, device=dev) if return_stats else None
        n = torch.empty(1, dtype=torch.int32, device=dev)
        nv.check(lib.xgtr_rollout(_stream(), C.byref(d), S, *args, top_k, top_p, nv.ptr(uniforms), temperature, nv.ptr(seq), nv.ptr(slp),
                                  nv.ptr(slq), nv.ptr(kept), nv.ptr(n), wp, wn), "xgtr_rollout")
        out = (seq, slp, slq, kept) if return_stats else (seq, slp)
        if not trim:
            return out + (n,)
        n = int(n.item())
        return tuple(o[:, :, :n] for o in out)

    def beam_captions(self, feats_rgb, feats_opfl, feat_mask, pos_feats, beam_size=5, suppress_token=1, return_trace=False):
        """The W = beam_size captions the model finds most likely for each of the B videos (include/xgate_beam.h: the search of
        beam.py / the reference's sample_beam, SAModel.py:129-161, as ONE enqueue with no host work per step).  Returns (seq
        (B,W,L) int64, seq_logp (B,W,L), score (B,W)[, trace (B,L,W,2) int32]); nothing here synchronises with the host.

        A video's beams come best first, each ranked by its summed log-probability `score` at the moment it finished; seq and
        seq_logp are zero after a beam's finish.  `suppress_token`: the word whose log-probability is lowered by 1000 before every
        merge (the reference does this for UNK, index 1); -1 turns it off.  `return_trace`: also the (token, parent slot) of every
        slot and step.  Eval mode, fp32 and device tensors only; beam_size may not exceed vocab_size or 8."""
        from . import _native_beam as nb
        inputs, W, sup = (feats_rgb, feats_opfl, feat_mask, pos_feats), int(beam_size), int(suppress_token)
        B, K, _, L, dev, d = self._search_open("beam_captions", inputs, False, beam=(W, sup))
        lib = nb.lib()
        args, wp, wn, keep = self._search_call("_beam_ws", (B, K, L, W, str(dev)), lambda: lib.xgcb_workspace_bytes(C.byref(d), W),
                                               "xgcb_workspace_bytes: invalid dims or too many rows (B %d, W %d)" % (B, W), inputs)
        seq = torch.empty(B, W, L, dtype=torch.int64, device=dev)
        seq_logp = torch.empty(B, W, L, dtype=torch.float32, device=dev)
        score = torch.empty(B, W, dtype=torch.float32, device=dev)
        trace = torch.empty(B, L, W, 2, dtype=torch.int32, device=dev) if return_trace else None
        nv.check(lib.xgcb_beam_search(_stream(), C.byref(d), W, sup, *args, nv.ptr(seq), nv.ptr(seq_logp), nv.ptr(score),
                                      nv.ptr(trace), wp, wn), "xgcb_beam_search")
        out = (seq, seq_logp, score)
        return out + (trace,) if return_trace else out

    def beam_captions_per_video(self, feats_rgb, feats_opfl, feat_mask, pos_feats, beam_size=5, suppress_token=1,
                                return_trace=False):
        """``beam_captions`` for S `pos_feats` rows per video on ONE encoder pass (include/xgate_beam_control.h): the B videos are
        handed over once, `pos_feats` is (B,S,R), and the result is what ``beam_captions`` gives on the batch with every video
        repeated S times, (video, template) pair by pair: (seq (B,S,W,L) int64, seq_logp (B,S,W,L), score (B,S,W)[, trace
        (B,S,L,W,2) int32]).  The encoder, init_hidden and v2a(V) run once per video, V and v2a(V) are not repeated and every
        step's attention reads them once per group of a video's S*W rows; one enqueue, nothing here synchronises with the host.

        `beam_size`, `suppress_token`, `return_trace` and the order of a pair's beams as in ``beam_captions``.  Eval mode, fp32 and
        device tensors only."""
        from . import _native_beam_control as nbc
        inputs, W, sup = (feats_rgb, feats_opfl, feat_mask, pos_feats), int(beam_size), int(suppress_token)
        B, K, S, L, dev, d = self._search_open("beam_captions_per_video", inputs, True, beam=(W, sup))
        lib = nbc.lib()
        args, wp, wn, keep = self._search_call("_beam_control_ws", (B, K, L, S, W, str(dev)),
                                               lambda: lib.xgbc_workspace_bytes(C.byref(d), S, W),
                                               "xgbc_workspace_bytes: invalid dims or too many rows (B %d, S %d, W %d)" % (B, S, W), inputs)
        seq = torch.empty(B, S, W, L, dtype=torch.int64, device=dev)
        seq_logp = torch.empty(B, S, W, L, dtype=torch.float32, device=dev)
        score = torch.empty(B, S, W, dtype=torch.float32, device=dev)
        trace = torch.empty(B, S, L, W, 2, dtype=torch.int32, device=dev) if return_trace else None
        nv.check(lib.xgbc_beam_search(_stream(), C.byref(d), S, W, sup, *args, nv.ptr(seq), nv.ptr(seq_logp), nv.ptr(score),
                                      nv.ptr(trace), wp, wn), "xgbc_beam_search")
        out = (seq, seq_logp, score)
        return out + (trace,) if return_trace else out

    def beam_captions_allowed(self, feats_rgb, feats_opfl, feat_mask, pos_feats, word_cat, allow, beam_size=5, suppress_token=1,
                              return_trace=False):
        """``beam_captions_per_video`` in which position t of a (video, template) pair's captions admits only words of the POS
        categories the pair allows there (include/xgate_beam_allow.h).  `word_cat` (V,) uint8: every word's category, below 32
        (``data.word_category_table``); `allow` (B,S,L) integers holding uint32 masks, bit c set = category c admitted
        (``control.allow_masks``; 0xFFFFFFFF: any word; a mask that admits no word of the vocabulary counts as that).  The softmax of
        a step runs over the allowed words alone and every other word is lowered by 1000 like the suppressed one, so every
        returned beam with a score above -500 holds allowed words only.  Returns what ``beam_captions_per_video`` returns; one
        enqueue, nothing here synchronises with the host.

        Raises as that method does, plus ValueError for a `word_cat` that is not (V,) uint8 or an `allow` that is not (B,S,L)
        integers.  Eval mode, fp32 and device tensors only."""
        from . import _native_beam_allow as nba
        name = "beam_captions_allowed"
        inputs, W, sup = (feats_rgb, feats_opfl, feat_mask, pos_feats), int(beam_size), int(suppress_token)
        self._search_gate(name)
        if not torch.is_tensor(word_cat) or word_cat.dtype != torch.uint8 or tuple(word_cat.shape) != (self.vocab_size,):
            raise ValueError("word_cat (V = %d,) uint8 expected, got %s" % (
                self.vocab_size, (tuple(word_cat.shape), word_cat.dtype) if torch.is_tensor(word_cat) else type(word_cat)))
        if not torch.is_tensor(allow) or allow.is_floating_point() or allow.is_complex() or allow.dtype == torch.bool:
            raise ValueError("allow holds integer masks")
        # (the constraint's own checks hold on any device: they come before the device gate of _search_open, behind the mode's)
        if pos_feats.dim() == 3 and tuple(allow.shape) != tuple(pos_feats.shape[:2]) + (self.seq_length,):
            raise ValueError("allow (B = %d, S = %d, L = %d) expected, got %s" % (pos_feats.shape[0], pos_feats.shape[1],
                                                                                  self.seq_length, tuple(allow.shape)))
        B, K, S, L, dev, d = self._search_open(name, inputs, True, beam=(W, sup))
        self._search_gate(name, word_cat, allow)
        with torch.no_grad():                        # the uint32 bit patterns in int32 storage
            a = allow.detach().long() & 0xFFFFFFFF
            a = torch.where(a >= 1 << 31, a - (1 << 32), a).to(torch.int32).contiguous()
            wc = word_cat.detach().contiguous()
        lib = nba.lib()
        args, wp, wn, keep = self._search_call("_beam_allow_ws", (B, K, L, S, W, str(dev)),
                                               lambda: lib.xgba_workspace_bytes(C.byref(d), S, W),
                                               "xgba_workspace_bytes: invalid dims or too many rows (B %d, S %d, W %d)" % (B, S, W), inputs)
        seq = torch.empty(B, S, W, L, dtype=torch.int64, device=dev)
        seq_logp = torch.empty(B, S, W, L, dtype=torch.float32, device=dev)
        score = torch.empty(B, S, W, dtype=torch.float32, device=dev)
        trace = torch.empty(B, S, L, W, 2, dtype=torch.int32, device=dev) if return_trace else None
        nv.check(lib.xgba_beam_search(_stream(), C.byref(d), S, W, sup, nv.ptr(wc), nv.ptr(a), *args, nv.ptr(seq), nv.ptr(seq_logp),
                                      nv.ptr(score), nv.ptr(trace), wp, wn), "xgba_beam_search")
        out = (seq, seq_logp, score)
        return out + (trace,) if return_trace else out

    def beam_captions_ruled(self, feats_rgb, feats_opfl, feat_mask, pos_feats, beam_size=5, suppress_token=1, no_repeat_ngram=0,
                            min_length=0, bad_endings=None, length_scale=None, word_cat=None, allow=None, return_trace=False):
        """``beam_captions_per_video`` -- with `word_cat` and `allow`, ``beam_captions_allowed`` -- under decoding rules
        (include/xgate_beam_rules.h, docs/CAPTION_RULES.md).  `no_repeat_ngram` = n >= 1: the word that would complete an n-gram a
        beam already holds is lowered by 1000 like the suppressed word, so no beam with a score above -500 holds an n-gram twice
        (0: off).  `min_length`: the end token 0 is lowered likewise at steps t < min_length.  `bad_endings`: up to 32 words (a
        sequence or tensor of indices, ``data.bad_ending_ids``) behind which the end token is lowered likewise.  `length_scale`
        (L,) in (0, 1] (``control.length_scale_table``): a (video, template) pair's finished beams are ranked by key = score *
        length_scale[step of the finish] instead of by score.  The log-sum-exp of a step is never changed by a ban: seq_logp stays
        the model's log-probability.  Returns (seq (B,S,W,L) int64, seq_logp (B,S,W,L), score (B,S,W), key (B,S,W)[, trace
        (B,S,L,W,2) int32]), a pair's beams in descending key; with every rule off seq, seq_logp, score and trace are those of the
        search without rules bit for bit and key == score.  One enqueue, no host work per step.

        Raises as ``beam_captions_per_video`` / ``beam_captions_allowed`` do, plus ValueError for n or `min_length` outside [0, L],
        L above 512, `bad_endings` outside [0, V) or more than 32 of them, a `length_scale` that is not (L,), not finite or outside
        (0, 1], and exactly one of `word_cat` / `allow` given.  `bad_endings` and `length_scale` are checked on the host: hand them
        over as host data (a device tensor is read back).  Eval mode, fp32 and device tensors only."""
        from . import _native_beam_rules as nbr
        name = "beam_captions_ruled"
        inputs, W, sup = (feats_rgb, feats_opfl, feat_mask, pos_feats), int(beam_size), int(suppress_token)
        self._search_gate(name)
        Ls, V = self.seq_length, self.vocab_size
        n, mn = int(no_repeat_ngram), int(min_length)
        # (the rules' own checks hold on any device: they come before the device gate of _search_open, behind the mode's)
        if Ls > nbr.XGBR_MAX_LENGTH:
            raise ValueError("seq_length <= %d expected, got %d" % (nbr.XGBR_MAX_LENGTH, Ls))
        if not 0 <= n <= Ls:
            raise ValueError("0 <= no_repeat_ngram <= seq_length = %d expected, got %d" % (Ls, n))
        if not 0 <= mn <= Ls:
            raise ValueError("0 <= min_length <= seq_length = %d expected, got %d" % (Ls, mn))
        bad = None
        if bad_endings is not None:
            bad = torch.as_tensor(bad_endings).detach().cpu()
            if bad.is_floating_point() or bad.is_complex() or bad.dtype == torch.bool or bad.dim() != 1:
                raise ValueError("bad_endings: a flat sequence of word indices expected")
            if bad.numel() > nbr.XGBR_MAX_BAD_END:
                raise ValueError("at most %d bad_endings expected, got %d" % (nbr.XGBR_MAX_BAD_END, bad.numel()))
            if bad.numel() and (int(bad.min()) < 0 or int(bad.max()) >= V):
                raise ValueError("bad_endings must lie in [0, vocab_size = %d)" % V)
            bad = bad.to(torch.int32).contiguous() if bad.numel() else None
        scale = None
        if length_scale is not None:
            scale = torch.as_tensor(length_scale).detach().cpu()
            if not scale.is_floating_point() or tuple(scale.shape) != (Ls,):
                raise ValueError("length_scale (L = %d,) floats expected, got %s" % (Ls, tuple(scale.shape)))
            scale = scale.to(torch.float32).contiguous()
            if not bool(torch.isfinite(scale).all()) or not bool(((scale > 0) & (scale <= 1)).all()):
                raise ValueError("every length_scale entry must be finite and lie in (0, 1]")
        if (word_cat is None) != (allow is None):
            raise ValueError("word_cat and allow come together: both or neither")
        if word_cat is not None:
            if not torch.is_tensor(word_cat) or word_cat.dtype != torch.uint8 or tuple(word_cat.shape) != (V,):
                raise ValueError("word_cat (V = %d,) uint8 expected, got %s" % (
                    V, (tuple(word_cat.shape), word_cat.dtype) if torch.is_tensor(word_cat) else type(word_cat)))
            if not torch.is_tensor(allow) or allow.is_floating_point() or allow.is_complex() or allow.dtype == torch.bool:
                raise ValueError("allow holds integer masks")
            if pos_feats.dim() == 3 and tuple(allow.shape) != tuple(pos_feats.shape[:2]) + (Ls,):
                raise ValueError("allow (B = %d, S = %d, L = %d) expected, got %s" % (pos_feats.shape[0], pos_feats.shape[1], Ls,
                                                                                      tuple(allow.shape)))
        B, K, S, L, dev, d = self._search_open(name, inputs, True, beam=(W, sup))
        a = wc = None
        if word_cat is not None:
            self._search_gate(name, word_cat, allow)
            with torch.no_grad():                    # the uint32 bit patterns in int32 storage
                a = allow.detach().long() & 0xFFFFFFFF
                a = torch.where(a >= 1 << 31, a - (1 << 32), a).to(torch.int32).contiguous()
                wc = word_cat.detach().contiguous()
        # the two small tables on the device, kept from the last call with the same values (no copy per call)
        tkey = (None if bad is None else tuple(bad.tolist()), None if scale is None else scale.numpy().tobytes(), str(dev))
        if getattr(self, "_beam_rules_tables", (None,))[0] != tkey:
            self._beam_rules_tables = (tkey, None if bad is None else bad.to(dev), None if scale is None else scale.to(dev))
        _, bad, scale = self._beam_rules_tables
        rules = nbr.XgBeamRules(n, mn, nv.ptr(bad), 0 if bad is None else bad.numel(), nv.ptr(scale))
        lib = nbr.lib()
        args, wp, wn, keep = self._search_call("_beam_rules_ws", (B, K, L, S, W, str(dev)),
                                               lambda: lib.xgbr_workspace_bytes(C.byref(d), S, W),
                                               "xgbr_workspace_bytes: invalid dims or too many rows (B %d, S %d, W %d)" % (B, S, W), inputs)
        seq = torch.empty(B, S, W, L, dtype=torch.int64, device=dev)
        seq_logp = torch.empty(B, S, W, L, dtype=torch.float32, device=dev)
        score = torch.empty(B, S, W, dtype=torch.float32, device=dev)
        key = torch.empty(B, S, W, dtype=torch.float32, device=dev)
        trace = torch.empty(B, S, L, W, 2, dtype=torch.int32, device=dev) if return_trace else None
        nv.check(lib.xgbr_beam_search(_stream(), C.byref(d), S, W, sup, C.byref(rules), nv.ptr(wc), nv.ptr(a), *args, nv.ptr(seq),
                                      nv.ptr(seq_logp), nv.ptr(score), nv.ptr(key), nv.ptr(trace), wp, wn), "xgbr_beam_search")
        out = (seq, seq_logp, score, key)
        return out + (trace,) if return_trace else out

    def beam_captions_diverse(self, feats_rgb, feats_opfl, feat_mask, pos_feats, groups, group_size, diversity=0.5, suppress_token=1,
                              return_trace=False):
        """Diverse beam search (include/xgate_beam_diverse.h) for S `pos_feats` rows per video on ONE encoder pass: per (video,
        template) pair Gd = groups beam searches of width Wg = group_size, a group steered away from the words the groups before
        it took at the same step by `diversity` (lambda >= 0) per live slot that took them.  `pos_feats` is (B,S,R).  Returns (seq
        (B,S,Gd,Wg,L) int64, seq_logp (B,S,Gd,Wg,L), score (B,S,Gd,Wg)[, trace (B,S,L,N,2) int32]), N = Gd Wg <= min(vocab_size, 8).

        A group's beams come best first, ranked by the PENALISED sum `score` at the moment they finished; seq_logp holds the
        unpenalised log-probabilities, so ``seq_logp.sum(-1)`` is the pure sum.  groups = 1 is ``beam_captions_per_video`` at
        beam_size = group_size bit for bit; the trace's parents are slot indices of the pair.  `suppress_token` and
        `return_trace` as in ``beam_captions``.  Eval mode, fp32 and device tensors only; one enqueue, nothing here synchronises
        with the host."""
        from . import _native_beam_diverse as ndb
        name = "beam_captions_diverse"
        inputs, sup = (feats_rgb, feats_opfl, feat_mask, pos_feats), int(suppress_token)
        self._search_gate(name)
        Gd, Wg, lam = int(groups), int(group_size), float(diversity)
        most = min(self.vocab_size, ndb.XGDB_MAX_BEAM)
        # (the search's own checks hold on any device: they come before the device gate of _search_open, behind the mode's)
        if Gd < 1 or Wg < 1 or Gd * Wg > most:
            raise ValueError("groups, group_size >= 1 and groups * group_size <= min(vocab_size = %d, %d) expected, got %d, %d"
                             % (self.vocab_size, ndb.XGDB_MAX_BEAM, Gd, Wg))
        if not (0.0 <= lam < float("inf")):
            raise ValueError("diversity must be finite and >= 0, got %r" % (diversity,))
        N = Gd * Wg
        B, K, S, L, dev, d = self._search_open(name, inputs, True, beam=(N, sup))
        lib = ndb.lib()
        args, wp, wn, keep = self._search_call("_beam_diverse_ws", (B, K, L, S, Gd, Wg, str(dev)),
                                               lambda: lib.xgdb_workspace_bytes(C.byref(d), S, Gd, Wg),
                                               "xgdb_workspace_bytes: invalid dims or too many rows (B %d, S %d, N %d)" % (B, S, N), inputs)
        seq = torch.empty(B, S, Gd, Wg, L, dtype=torch.int64, device=dev)
        seq_logp = torch.empty(B, S, Gd, Wg, L, dtype=torch.float32, device=dev)
        score = torch.empty(B, S, Gd, Wg, dtype=torch.float32, device=dev)
        trace = torch.empty(B, S, L, N, 2, dtype=torch.int32, device=dev) if return_trace else None
        nv.check(lib.xgdb_beam_search(_stream(), C.byref(d), S, Gd, Wg, lam, sup, *args, nv.ptr(seq), nv.ptr(seq_logp), nv.ptr(score),
                                      nv.ptr(trace), wp, wn), "xgdb_beam_search")
        out = (seq, seq_logp, score)
        return out + (trace,) if return_trace else out

    def score_captions_per_video(self, feats_rgb, feats_opfl, feat_mask, pos_feats, captions, cross=False):
        """The log-probability the captioner gives GIVEN captions, on ONE encoder pass (include/xgate_score.h): the B videos are
        handed over once, `pos_feats` is (B,S,R) and `captions` (B,N,L') integer tokens with L' <= seq_length, zero = EOS (padded
        with zeros to L = seq_length on their own device).  A row's result is what ``sample`` with `forced_tokens` gives on the
        batch with every video repeated per row: tok_logp, the untempered log-probability of token j at step j in the COUNTED
        columns -- column 0 and every column whose preceding tokens are all non-zero; the first EOS is counted -- and 0 elsewhere;
        count (int32), the number of counted columns; score, the sum of tok_logp.

        cross=False: caption s is scored under template s (N == S) -> (tok_logp (B,S,L), score (B,S), count (B,S)).
        cross=True: every caption under every template, rows ordered (b, s, n) -> (B,S,N,L), (B,S,N), (B,S,N).

        Eval mode, fp32 and device tensors only; one enqueue, nothing here synchronises with the host, token values are clamped
        into [0, vocab_size) by the kernels and nothing returned carries an autograd graph."""
        from . import _native_score as nsc
        inputs = (feats_rgb, feats_opfl, feat_mask, pos_feats)
        # the captions' own checks come before the device gate of _search_open (they hold on any device), behind the mode's
        self._search_gate("score_captions_per_video")
        cap, B, L = captions, feats_rgb.shape[0], self.seq_length
        if not torch.is_tensor(cap) or cap.is_floating_point() or cap.is_complex() or cap.dtype == torch.bool:
            raise ValueError("captions are integer tokens")
        if cap.dim() != 3 or cap.shape[0] != B or cap.shape[1] < 1:
            raise ValueError("captions (B = %d, N, L') expected, got %s" % (B, tuple(cap.shape)))
        N = int(cap.shape[1])
        if cap.shape[2] > L:
            raise ValueError("captions have %d tokens, seq_length is %d" % (cap.shape[2], L))
        if not cross and pos_feats.dim() == 3 and N != pos_feats.shape[1]:
            raise ValueError("%d captions per video for %d templates: N == S expected (cross=True scores every caption under every "
                             "template)" % (N, pos_feats.shape[1]))
        B, K, S, L, dev, d = self._search_open("score_captions_per_video", inputs, True)
        self._search_gate("score_captions_per_video", cap)
        with torch.no_grad():
            cap = torch.nn.functional.pad(cap.detach().long(), (0, L - cap.shape[2]))
            pos = pos_feats.detach()
            if cross:                                    # rows (b, s, n): template s with caption n
                pos = pos.unsqueeze(2).expand(B, S, N, pos.shape[2]).reshape(B, S * N, pos.shape[2])
                cap = cap.unsqueeze(1).expand(B, S, N, L).reshape(B, S * N, L)
            cap = cap.contiguous()
        Q = S * N if cross else S
        lib = nsc.lib()
        args, wp, wn, keep = self._search_call("_score_ws", (B, K, L, Q, str(dev)), lambda: lib.xgsc_workspace_bytes(C.byref(d), Q),
                                               "xgsc_workspace_bytes: invalid dims or too many rows (B %d, Q %d)" % (B, Q),
                                               inputs[:3] + (pos,))
        shape = (B, S, N) if cross else (B, S)
        tok_logp = torch.empty(*shape, L, dtype=torch.float32, device=dev)
        score = torch.empty(*shape, dtype=torch.float32, device=dev)
        count = torch.empty(*shape, dtype=torch.int32, device=dev)
        nv.check(lib.xgsc_score_captions(_stream(), C.byref(d), Q, *args, nv.ptr(cap), nv.ptr(tok_logp), nv.ptr(score), nv.ptr(count),
                                         wp, wn), "xgsc_score_captions")
        return tok_logp, score, count


# ====================================================================== autograd glue
def _grads_struct(model, device=None):
    """model._grads_struct() under the name callers outside this module import: (g, struct of gradient pointers)."""
    return model._grads_struct()


def _take_workspace(model, d, dev, save):
    """(ws, pointer, bytes) of a forward's workspace: its own until the backward has run when it saves activations,
    else the shared scratch."""
    ws = model._pool.take(d, dev) if save else model._pool.shared(d, dev)
    return (ws,) + _ws_ptr(ws)


def _open_backward(ctx):
    """What every backward hands the library, from what its forward left in ctx (model, d, keep, ws, run):
    (model, d, g, gs, b, keep, wp, wn, ps, run) -- g / gs of _grads_struct, run with the gradient event."""
    model = ctx.model
    g, gs = model._grads_struct()
    b, keep = model._batch(*ctx.keep)
    wp, wn = _ws_ptr(ctx.ws)
    return model, ctx.d, g, gs, b, keep, wp, wn, model._params_struct(), _with_grad_event(model, ctx.run)


def _close_backward(ctx, g, k):
    """Give the forward's workspace back and return backward's result: None for the k non-parameter inputs, then the
    parameters' gradient views (None each when the library added into the bound gradient buffer)."""
    ctx.model._pool.give(ctx.d, ctx.keep[0].device, ctx.ws)
    ctx.ws = None
    return (None,) * k + tuple(ctx.model._grad_views(g))


def _wants_dpos(model, pos_feats, name):
    """Whether this call of a fused loss has to return the gradient of pos_feats (joint training, docs/JOINT_TRAINING.md)."""
    if not (torch.is_tensor(pos_feats) and pos_feats.requires_grad and torch.is_grad_enabled()):
        return False
    if model.precision == "bf16":
        raise NotImplementedError('%s: the gradient of pos_feats is not implemented under precision = "bf16" (fp32 and bf16x3 '
                                  'are): detach pos_feats or choose another precision' % name)
    return True


def _caption_dpos(ctx, form, Q, d, b, run, wp, wn, pos_index, out):
    """`out` (backward's result) with the gradient of pos_feats at `pos_index` when the forward's pos_feats required one:
    xgj_caption_dpos behind the fused-loss backward that has just been enqueued on this stream and workspace.  Otherwise `out`
    as it is, and nothing runs."""
    if not ctx.needs_input_grad[pos_index]:
        return out
    from . import _native_joint as nj
    shape, dtype = ctx.pos_meta
    dpos = torch.empty(shape, dtype=torch.float32, device=ctx.keep[0].device)
    nv.check(nj.lib().xgj_caption_dpos(_stream(), C.byref(d), Q, form, C.byref(b), C.byref(run), wp, wn, nv.ptr(dpos)),
             "xgj_caption_dpos")
    return out[:pos_index] + (dpos.to(dtype),) + out[pos_index + 1:]


def _rollout_backward(ctx, dslp, k):
    """xg_rollout_bwd of the sampled rollout whose activations ctx.ws holds: backward of both rollout functions (k: the
    number of their non-parameter inputs)."""
    if not ctx.need_grad:
        raise nv.XgError("rollout ran without saved activations")
    model, d, g, gs, b, keep, wp, wn, ps, run = _open_backward(ctx)
    full = torch.zeros(d.B, d.T - 1, dtype=torch.float32, device=keep[0].device)
    full[:, :dslp.shape[1]] = dslp
    nv.check(nv.lib().xg_rollout_bwd(_stream(), C.byref(d), C.byref(ps), C.byref(gs), C.byref(b), C.byref(run),
                                     wp, wn, nv.ptr(full)), "xg_rollout_bwd")
    return _close_backward(ctx, g, k)


class _XEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, save, ss, feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, *params):
        B, K, _ = feats_rgb.shape
        T = seq.shape[1]
        dev = feats_rgb.device
        d = model._dims(B, K, T)
        ws, wp, wn = _take_workspace(model, d, dev, save)
        b, keep = model._batch(feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask)
        logp = torch.empty(B, T, model.vocab_size, dtype=torch.float32, device=dev)
        cat = torch.empty(B, T, model.category_size, dtype=torch.float32, device=dev)
        ps, bn, run = model._params_struct(), model._bn_struct(), model._run(save)
        if ss is None:
            nv.check(nv.lib().xg_forward_xe(_stream(), C.byref(d), C.byref(ps), C.byref(bn), C.byref(b), C.byref(run),
                                            wp, wn, nv.ptr(logp), nv.ptr(cat)), "xg_forward_xe")
        else:
            nv.check(nv.lib().xg_forward_ss(_stream(), C.byref(d), C.byref(ps), C.byref(bn), C.byref(b), C.byref(run),
                                            ss[0], nv.ptr(ss[1]), nv.ptr(ss[2]), wp, wn, nv.ptr(logp), nv.ptr(cat)),
                     "xg_forward_ss")
        model._bump_bn()
        ctx.model, ctx.d, ctx.ws, ctx.keep, ctx.run, ctx.saved_ws, ctx.ss = model, d, ws, keep, run, save, ss is not None
        return logp, cat

    @staticmethod
    def backward(ctx, dlogp, dcat):
        if not ctx.saved_ws:
            raise nv.XgError("backward without saved activations")
        model, d, g, gs, b, keep, wp, wn, ps, run = _open_backward(ctx)
        dl = None if dlogp is None else dlogp.contiguous().float()
        dc = None if dcat is None else dcat.contiguous().float()
        fn = nv.lib().xg_backward_ss if ctx.ss else nv.lib().xg_backward_xe
        nv.check(fn(_stream(), C.byref(d), C.byref(ps), C.byref(gs), C.byref(b), C.byref(run),
                    wp, wn, nv.ptr(dl), nv.ptr(dc)), "xg_backward_ss" if ctx.ss else "xg_backward_xe")
        return _close_backward(ctx, g, 9)


class _XELossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, save, feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes, class_mask,
                weight_class, *params):
        B, K, _ = feats_rgb.shape
        T = seq.shape[1]
        dev = feats_rgb.device
        d = model._dims(B, K, T)
        ws, wp, wn = _take_workspace(model, d, dev, save)
        b, keep = model._batch(feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask)
        cc = None if cap_classes is None else cap_classes.detach().contiguous().long()
        cm = None if class_mask is None else class_mask.detach().contiguous().float()
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        ps, bn, run = model._params_struct(), model._bn_struct(), model._run(save)
        # (the counters' increment is independent of the forward: enqueued in FRONT of it, it is not one more small launch on the
        #  main stream between the loss and the start of the backward)
        model._bump_bn()
        try:
            nv.check(nv.lib().xg_xe_loss_fwd(_stream(), C.byref(d), C.byref(ps), C.byref(bn), C.byref(b), nv.ptr(cc),
                                             nv.ptr(cm), weight_class, C.byref(run), wp, wn, nv.ptr(losses)), "xg_xe_loss_fwd")
        except Exception:
            model._bump_bn(-1)                     # the call was refused: num_batches_tracked stays where it was
            raise
        ctx.model, ctx.d, ctx.ws, ctx.keep, ctx.run, ctx.saved_ws = model, d, ws, keep, run, save
        ctx.cc, ctx.cm, ctx.wc = cc, cm, weight_class
        ctx.pos_meta = (tuple(pos_feats.shape), pos_feats.dtype)
        model.last_losses = losses.detach()        # READ-ONLY for callers: it shares storage with the returned loss (no copy kernel)
        return losses[0]                           # (a view of the three-element result: no copy kernel)

    @staticmethod
    def backward(ctx, dloss):
        model, d, g, gs, b, keep, wp, wn, ps, run = _open_backward(ctx)
        dl = dloss.detach().contiguous().float().to(keep[0].device)
        nv.check(nv.lib().xg_xe_loss_bwd(_stream(), C.byref(d), C.byref(ps), C.byref(gs), C.byref(b), nv.ptr(ctx.cc),
                                         nv.ptr(ctx.cm), ctx.wc, nv.ptr(dl), C.byref(run), wp, wn), "xg_xe_loss_bwd")
        # (before the workspace goes back to the pool: the sum reads what the backward left in it)
        from . import _native_joint as nj
        extra = _caption_dpos(ctx, nj.XGJ_FORM_XE, 0, d, b, run, wp, wn, 5, (None,) * 11)
        return extra + _close_backward(ctx, g, 0)


class _XELossVideoFunction(torch.autograd.Function):
    """_XELossFunction with the B videos once and Q caption rows each (include/xgate_train_video.h)."""

    @staticmethod
    def forward(ctx, model, save, feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes, class_mask,
                weight_class, *params):
        from . import _native_train_video as ntv
        B, K, _ = feats_rgb.shape
        Q, T = seq.shape[1], seq.shape[2]
        dev = feats_rgb.device
        d = model._dims(B, K, T)
        key, ws = model._video_workspace(d, Q, dev, save)
        wp, wn = _ws_ptr(ws)
        rows = (pos_feats.reshape(B * Q, -1), seq.reshape(B * Q, T), seq_mask.reshape(B * Q, T))
        b, keep = model._batch(feats_rgb, feats_opfl, feat_mask, *rows)
        cc = None if cap_classes is None else cap_classes.detach().reshape(B * Q, T).contiguous().long()
        cm = None if class_mask is None else class_mask.detach().reshape(B * Q, T).contiguous().float()
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        ps, bn, run = model._params_struct(), model._bn_struct(), model._run(save)
        model._bump_bn()                           # (in FRONT of the forward, as _XELossFunction has it)
        try:
            nv.check(ntv.lib().xgtv_xe_loss_fwd(_stream(), C.byref(d), Q, C.byref(ps), C.byref(bn), C.byref(b), nv.ptr(cc), nv.ptr(cm),
                                                weight_class, C.byref(run), wp, wn, nv.ptr(losses)), "xgtv_xe_loss_fwd")
        except Exception:
            model._bump_bn(-1)                     # the call was refused: num_batches_tracked stays where it was
            if save:
                model._video_pool[(key, True)].append(ws)
            raise
        ctx.model, ctx.d, ctx.Q, ctx.ws, ctx.key, ctx.keep, ctx.run, ctx.saved_ws = model, d, Q, ws, key, keep, run, save
        ctx.cc, ctx.cm, ctx.wc = cc, cm, weight_class
        ctx.pos_meta = (tuple(pos_feats.shape), pos_feats.dtype)
        model.last_losses = losses.detach()        # READ-ONLY for callers: it shares storage with the returned loss (no copy kernel)
        return losses[0]

    @staticmethod
    def backward(ctx, dloss):
        from . import _native_train_video as ntv
        if not ctx.saved_ws:
            raise nv.XgError("backward without saved activations")
        model = ctx.model
        g, gs = model._grads_struct()
        b, keep = model._batch(*ctx.keep)
        wp, wn = _ws_ptr(ctx.ws)
        run = _with_grad_event(model, ctx.run)
        dl = dloss.detach().contiguous().float().to(keep[0].device)
        nv.check(ntv.lib().xgtv_xe_loss_bwd(_stream(), C.byref(ctx.d), ctx.Q, C.byref(model._params_struct()), C.byref(gs), C.byref(b),
                                            nv.ptr(ctx.cc), nv.ptr(ctx.cm), ctx.wc, nv.ptr(dl), C.byref(run), wp, wn),
                 "xgtv_xe_loss_bwd")
        from . import _native_joint as nj
        extra = _caption_dpos(ctx, nj.XGJ_FORM_VIDEO, ctx.Q, ctx.d, b, run, wp, wn, 5, (None,) * 11)
        model._video_pool[(ctx.key, True)].append(ctx.ws)
        model._last_video_ws = (ctx.d, ctx.Q, ctx.ws)      # tests / tools: what xgtv_video_grads reads (valid until the next call reuses it)
        ctx.ws = None
        return extra + tuple(model._grad_views(g))


class _XELossSSFunction(torch.autograd.Function):
    """The fused loss under scheduled sampling (include/xgate_ss.h).  Q == 0: _XELossFunction's shapes and workspace pool;
    Q >= 1: _XELossVideoFunction's shapes, a pool of its own sizes.  The fed tokens go to model.last_ss_tokens."""

    @staticmethod
    def forward(ctx, model, save, Q, ss_prob, u, feats_rgb, feats_opfl, feat_mask, pos_feats, seq, seq_mask, cap_classes, class_mask,
                weight_class, *params):
        from . import _native_ss as nss
        B, K, _ = feats_rgb.shape
        T = seq.shape[-1]
        M = B * max(Q, 1)
        dev = feats_rgb.device
        d = model._dims(B, K, T)
        if Q == 0:
            key = None
            ws, wp, wn = _take_workspace(model, d, dev, save)
        else:
            key, ws = model._ss_video_workspace(d, Q, dev, save)
            wp, wn = _ws_ptr(ws)
        b, keep = model._batch(feats_rgb, feats_opfl, feat_mask, pos_feats.reshape(M, -1), seq.reshape(M, T), seq_mask.reshape(M, T))
        cc = None if cap_classes is None else cap_classes.detach().reshape(M, T).contiguous().long()
        cm = None if class_mask is None else class_mask.detach().reshape(M, T).contiguous().float()
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        tok = torch.empty(T, M, dtype=torch.int64, device=dev)
        ps, bn, run = model._params_struct(), model._bn_struct(), model._run(save)

        def give_back():
            if Q == 0:
                if save:
                    model._pool.give(d, dev, ws)
            elif save:
                model._ss_video_pool[(key, True)].append(ws)

        model._bump_bn()                           # (in FRONT of the forward, as _XELossFunction has it)
        try:
            nv.check(nss.lib().xgss_xe_loss_fwd(_stream(), C.byref(d), Q, C.byref(ps), C.byref(bn), C.byref(b), nv.ptr(cc), nv.ptr(cm),
                                                weight_class, ss_prob, nv.ptr(u[0]), nv.ptr(u[1]), C.byref(run), wp, wn,
                                                nv.ptr(losses), nv.ptr(tok)), "xgss_xe_loss_fwd")
        except Exception:
            model._bump_bn(-1)                     # the call was refused: num_batches_tracked stays where it was
            give_back()
            raise
        ctx.model, ctx.d, ctx.Q, ctx.ws, ctx.key, ctx.keep, ctx.run, ctx.saved_ws = model, d, Q, ws, key, keep, run, save
        ctx.cc, ctx.cm, ctx.wc = cc, cm, weight_class
        ctx.pos_meta = (tuple(pos_feats.shape), pos_feats.dtype)
        model.last_losses = losses.detach()        # READ-ONLY for callers: it shares storage with the returned loss (no copy kernel)
        model.last_ss_tokens = tok
        return losses[0]

    @staticmethod
    def backward(ctx, dloss):
        from . import _native_ss as nss
        if not ctx.saved_ws:
            raise nv.XgError("backward without saved activations")
        model = ctx.model
        g, gs = model._grads_struct()
        b, keep = model._batch(*ctx.keep)
        wp, wn = _ws_ptr(ctx.ws)
        run = _with_grad_event(model, ctx.run)
        dl = dloss.detach().contiguous().float().to(keep[0].device)
        nv.check(nss.lib().xgss_xe_loss_bwd(_stream(), C.byref(ctx.d), ctx.Q, C.byref(model._params_struct()), C.byref(gs), C.byref(b),
                                            nv.ptr(ctx.cc), nv.ptr(ctx.cm), ctx.wc, nv.ptr(dl), C.byref(run), wp, wn),
                 "xgss_xe_loss_bwd")
        from . import _native_joint as nj
        extra = _caption_dpos(ctx, nj.XGJ_FORM_SS, ctx.Q, ctx.d, b, run, wp, wn, 8, (None,) * 14)
        if ctx.Q == 0:
            model._pool.give(ctx.d, keep[0].device, ctx.ws)
        else:
            model._ss_video_pool[(ctx.key, True)].append(ctx.ws)
        model._last_ss_ws = ctx.ws                 # tests: the workspace the call ran in (valid until the next call reuses it)
        ctx.ws = None
        return extra + tuple(model._grad_views(g))


class _RolloutVideoFunction(torch.autograd.Function):
    """The sampled rollout with the B videos once and S rollout rows each (include/xgate_scst_video.h), modelled on
    _XELossVideoFunction: a workspace of its own pool, given back after the backward and when the call is refused."""

    @staticmethod
    def forward(ctx, model, save, feats_rgb, feats_opfl, feat_mask, pos_feats, uniforms, temperature, *params):
        from . import _native_scst_video as nsv
        B, K, _ = feats_rgb.shape
        S, L = pos_feats.shape[1], model.seq_length
        dev = feats_rgb.device
        d = model._dims(B, K, L + 1)
        key, ws = model._scst_video_workspace(d, S, dev, save)
        wp, wn = _ws_ptr(ws)
        b, keep = model._batch(feats_rgb, feats_opfl, feat_mask, pos_feats.reshape(B * S, -1))
        if uniforms is None:
            uniforms = torch.rand(L + 1, B * S, device=dev, dtype=torch.float32)
        uniforms = uniforms.detach().contiguous().float()
        seq = torch.empty(B, S, L, dtype=torch.int64, device=dev)
        slp = torch.empty(B, S, L, dtype=torch.float32, device=dev)
        n = torch.empty(1, dtype=torch.int32, device=dev)
        ps, bn, run = model._params_struct(), model._bn_struct(), model._run(save)
        model._bump_bn()                           # (in FRONT of the forward, as _XELossFunction has it)
        try:
            nv.check(nsv.lib().xgsv_rollout(_stream(), C.byref(d), S, C.byref(ps), C.byref(bn), C.byref(b), C.byref(run),
                                            nv.ptr(uniforms), temperature, nv.ptr(seq), nv.ptr(slp), nv.ptr(n), wp, wn),
                     "xgsv_rollout")
        except Exception:
            model._bump_bn(-1)                     # the call was refused: num_batches_tracked stays where it was
            if save:
                model._scst_video_pool[(key, True)].append(ws)
            raise
        ctx.model, ctx.d, ctx.S, ctx.ws, ctx.key, ctx.keep, ctx.run, ctx.saved_ws = model, d, S, ws, key, keep, run, save
        ctx.mark_non_differentiable(seq, n)
        return seq, slp, n

    @staticmethod
    def backward(ctx, dseq, dslp, dn):
        from . import _native_scst_video as nsv
        if not ctx.saved_ws:
            raise nv.XgError("backward without saved activations")
        model, d, S = ctx.model, ctx.d, ctx.S
        g, gs = model._grads_struct()
        b, keep = model._batch(*ctx.keep)
        wp, wn = _ws_ptr(ctx.ws)
        run = _with_grad_event(model, ctx.run)
        L = d.T - 1
        full = dslp.detach().reshape(d.B * S, -1).float()
        if full.shape[1] != L:                     # (a gradient of trimmed log-probs: the columns behind n carry none)
            wide = torch.zeros(d.B * S, L, dtype=torch.float32, device=keep[0].device)
            wide[:, :full.shape[1]] = full
            full = wide
        full = full.contiguous()
        nv.check(nsv.lib().xgsv_rollout_bwd(_stream(), C.byref(d), S, C.byref(model._params_struct()), C.byref(gs), C.byref(b),
                                            C.byref(run), nv.ptr(full), wp, wn), "xgsv_rollout_bwd")
        model._scst_video_pool[(ctx.key, True)].append(ctx.ws)
        model._last_scst_video_ws = (d, S, ctx.ws)         # tests / tools (valid until the next call reuses it)
        ctx.ws = None
        return (None,) * 8 + tuple(model._grad_views(g))


class _RolloutFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, feats_rgb, feats_opfl, feat_mask, pos_feats, mode, uniforms, forced, temperature,
                need_grad, bn_update, *params):
        B, K, _ = feats_rgb.shape
        T = model.seq_length + 1
        dev = feats_rgb.device
        d = model._dims(B, K, T)
        ws, wp, wn = _take_workspace(model, d, dev, need_grad)
        b, keep = model._batch(feats_rgb, feats_opfl, feat_mask, pos_feats)
        seq = torch.zeros(B, T - 1, dtype=torch.int64, device=dev)
        slp = torch.zeros(B, T - 1, dtype=torch.float32, device=dev)
        n = torch.zeros(1, dtype=torch.int32, device=dev)
        if mode == nv.XG_ROLLOUT_SAMPLE and uniforms is None:
            uniforms = torch.rand(T, B, device=dev, dtype=torch.float32)
        if uniforms is not None:
            uniforms = uniforms.detach().contiguous().float()
        if forced is not None:
            f = torch.zeros(B, T - 1, dtype=torch.int64, device=dev)
            f[:, :forced.shape[1]] = forced.to(dev)
            forced = f
        ps, bn, run = model._params_struct(), model._bn_struct(), model._run(need_grad)
        if not bn_update and model.training:   # batch statistics are used, the running buffers are left alone
            bn = nv.XgBnState()
        nv.check(nv.lib().xg_rollout(_stream(), C.byref(d), C.byref(ps), C.byref(bn), C.byref(b), C.byref(run), mode,
                                     nv.ptr(uniforms), nv.ptr(forced), temperature, wp, wn, nv.ptr(seq), nv.ptr(slp),
                                     nv.ptr(n)), "xg_rollout")
        if bn_update:
            model._bump_bn()
        ctx.model, ctx.d, ctx.ws, ctx.keep, ctx.run, ctx.need_grad = model, d, ws, keep, run, need_grad
        ctx.mark_non_differentiable(seq, n)
        if not need_grad:
            ctx.mark_non_differentiable(slp)
        return seq, slp, n

    @staticmethod
    def backward(ctx, dseq, dslp, dn):
        return _rollout_backward(ctx, dslp, 11)


class _RolloutPairFunction(torch.autograd.Function):
    """Sampled rollout + greedy baseline of one SCST iteration as ONE batch of 2m rows (xg_rollout_pair); the sampled
    half's activations are compacted into an m-row workspace, so backward is xg_rollout_bwd of the sampled rollout alone.
    two_seeds (train-mode dropout): a dropout seed per half (xgpr_rollout_pair_videos, include/xgate_pair.h); the backward is the
    same one, since the sampled rows keep the first seed and the element indices of an m-row call.
    Returns (gen, sample_logprobs, greedy, n, greedy_logprobs)."""

    @staticmethod
    def forward(ctx, model, feats_rgb, feats_opfl, feat_mask, pos_feats, uniforms, temperature, need_grad, two_seeds, *params):
        B, K, _ = feats_rgb.shape
        T = model.seq_length + 1
        dev = feats_rgb.device
        d1, d2 = model._dims(B, K, T), model._dims(2 * B, K, T)
        ws2 = model._pool.shared(d2, dev)
        wp2, wn2 = _ws_ptr(ws2)
        # the videos are handed over ONCE: the library runs the encoder on the m-row batch and repeats V / v2a(V) / the
        # initial state on the device (xg_rollout_pair_videos) -- no torch.cat of the inputs, half the encoder work
        fm = feat_mask
        if fm.dim() == 1:
            fm = fm.unsqueeze(0).expand(B, K)
        b1, keep1 = model._batch(feats_rgb, feats_opfl, fm, pos_feats)
        seq = torch.zeros(2 * B, T - 1, dtype=torch.int64, device=dev)
        slp = torch.zeros(2 * B, T - 1, dtype=torch.float32, device=dev)
        n = torch.zeros(2, dtype=torch.int32, device=dev)
        if uniforms is None:
            uniforms = torch.rand(T, B, device=dev, dtype=torch.float32)
        uniforms = uniforms.detach().contiguous().float()
        ps, bn, run = model._params_struct(), model._bn_struct(), model._run(need_grad)
        # rollout + compaction of the sampled half into the m-row workspace (what the backward reads) as one call: the encoder
        # runs there in the first place, and the sampled rows' logits are written there by the rollout itself
        ws1, wp1, wn1 = _take_workspace(model, d1, dev, need_grad)
        tail = (nv.ptr(uniforms), temperature, wp2, wn2, C.byref(d1), wp1, wn1, 1 if need_grad else 0, nv.ptr(seq), nv.ptr(slp), nv.ptr(n))
        head = (_stream(), C.byref(d2), C.byref(ps), C.byref(bn), C.byref(b1), C.byref(run))
        if two_seeds:
            # the greedy call's seed: the NEXT one of the model's counter, as when the two rollouts run as two calls (sampled first)
            from . import _native_pair as npr
            nv.check(npr.lib().xgpr_rollout_pair_videos(*head, model._run(False).seed, *tail), "xgpr_rollout_pair_videos")
        else:
            nv.check(nv.lib().xg_rollout_pair_videos(*head, *tail), "xg_rollout_pair_videos")
        if not need_grad:
            ws1 = None
        model._bump_bn(2)                         # two sample() calls of the reference: two running-statistics updates (in the library)
        ctx.model, ctx.d, ctx.ws, ctx.run, ctx.need_grad = model, d1, ws1, run, need_grad
        ctx.keep = (feats_rgb, feats_opfl, feat_mask, pos_feats)
        gen, greedy = seq[:B], seq[B:]
        slp_s, slp_g = slp[:B], slp[B:]
        ctx.mark_non_differentiable(gen, greedy, n, slp_g)
        if not need_grad:
            ctx.mark_non_differentiable(slp_s)
        return gen, slp_s, greedy, n, slp_g

    @staticmethod
    def backward(ctx, dgen, dslp, dgreedy, dn, dglp):
        return _rollout_backward(ctx, dslp, 9)


# ====================================================================== criteria
class _NLLFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, target, mask, mask2, roll):
        B, T, V = logp.shape
        logp = logp.contiguous()
        target = target.detach().contiguous().long()
        mask = mask.detach().contiguous().float()
        m2 = None if mask2 is None else mask2.detach().contiguous().float()
        sums = torch.empty(2, dtype=torch.float32, device=logp.device)
        nv.check(nv.lib().xg_nll_fwd(_stream(), nv.ptr(logp), nv.ptr(target), nv.ptr(mask), nv.ptr(m2), B, T, V, roll,
                                     nv.ptr(sums)), "xg_nll_fwd")
        ctx.meta = (B, T, V, roll, target, mask, m2, sums)
        return sums[0] / sums[1]

    @staticmethod
    def backward(ctx, dloss):
        B, T, V, roll, target, mask, m2, sums = ctx.meta
        dlogp = torch.empty(B, T, V, dtype=torch.float32, device=sums.device)
        dl = dloss.detach().reshape(1).contiguous().float().to(sums.device)      # device scalar: no sync, no extra pass
        nv.check(nv.lib().xg_nll_bwd(_stream(), nv.ptr(target), nv.ptr(mask), nv.ptr(m2), B, T, V, roll, nv.ptr(sums),
                                     1.0, nv.ptr(dl), nv.ptr(dlogp)), "xg_nll_bwd")
        return dlogp, None, None, None, None


class LanguageModelCriterion(nn.Module):
    """reference caption_src/SAModel.py:221-234: masked NLL with the target rolled left by one."""

    def forward(self, input, target, mask):
        return _NLLFunction.apply(input, target, mask, None, 1)


class ClassiferCriterion(nn.Module):
    """reference caption_src/SAModel.py:236-253: masked NLL, target not rolled, optional class mask."""

    def forward(self, input, target, mask, class_mask=None):
        return _NLLFunction.apply(input, target, mask, class_mask, 0)


class _RewardFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, slp, seq, reward, n):
        m, L = slp.shape
        slp_c = slp if slp.stride(1) == 1 else slp.contiguous()
        seq = seq.detach()
        seq = seq if (seq.stride(1) == 1 and seq.dtype == torch.int64) else seq.contiguous().long()
        reward = reward.detach()
        reward = reward.float() if reward.dtype != torch.float32 else reward
        if reward.dim() == 0:                  # one scalar for every element (broadcast like the reference's input * reward)
            reward = reward.reshape(1, 1)
        if reward.dim() == 1:
            # The reference flattens both tensors (SAModel.py:260-261: view(-1)) and never broadcasts, so a 1-D reward has no
            # reference meaning unless it is the full m*L vector.  Extensions: (m*L,) is the flattened (m, L) matrix; (1,) one
            # value for all; (m,) with m != L one value per video; (L,) with L != m one value per position.  m == L is ambiguous
            # and rejected -- pass (m, 1) or (1, L).
            k = reward.shape[0]
            if k == m * L and m > 1 and L > 1:
                reward = reward.reshape(m, L)
            elif k == 1:
                reward = reward.reshape(1, 1)
            elif m == L and k == m:
                raise nv.XgError("1-D reward of length m == L is ambiguous: pass (m, 1) per video or (1, L) per position")
            elif k == m:
                reward = reward.unsqueeze(1)
            elif k == L:
                reward = reward.unsqueeze(0)
            else:
                raise nv.XgError("1-D reward must have m, L or m*L elements")
        if reward.shape[0] not in (1, m):
            raise nv.XgError("reward must broadcast against the (m, L) log-probs")
        if reward.shape[1] == 1:
            rs_b, rs_t = (reward.stride(0) if reward.shape[0] == m else 0), 0
        else:
            if reward.shape[1] < L:
                raise nv.XgError("reward has fewer columns than the log-probs")
            rs_b, rs_t = (reward.stride(0) if reward.shape[0] == m else 0), reward.stride(1)
        nd = None if n is None else n.detach().reshape(-1)[:1].to(torch.int32)
        sums = torch.empty(2, dtype=torch.float32, device=slp.device)
        nv.check(nv.lib().xg_reward_fwd(_stream(), nv.ptr(slp_c), slp_c.stride(0), nv.ptr(seq), seq.stride(0), nv.ptr(reward),
                                        rs_b, rs_t, nv.ptr(nd), m, L, nv.ptr(sums)), "xg_reward_fwd")
        ctx.meta = (m, L, seq, reward, rs_b, rs_t, nd, sums)
        return sums[0] / sums[1]

    @staticmethod
    def backward(ctx, dloss):
        m, L, seq, reward, rs_b, rs_t, nd, sums = ctx.meta
        dslp = torch.empty(m, L, dtype=torch.float32, device=sums.device)
        dl = dloss.detach().reshape(1).contiguous().float().to(sums.device)
        nv.check(nv.lib().xg_reward_bwd(_stream(), nv.ptr(seq), seq.stride(0), nv.ptr(reward), rs_b, rs_t, nv.ptr(nd), m, L,
                                        nv.ptr(sums), nv.ptr(dl), nv.ptr(dslp), L), "xg_reward_bwd")
        return dslp, None, None, None


class RewardCriterion(nn.Module):
    """reference caption_src/SAModel.py:255-267: policy-gradient loss -sum(input * reward * mask) / sum(mask) with
    mask[:, 0] = 1, mask[:, t] = seq[:, t-1] > 0, as ONE HIP launch forward and one backward (xg_reward_fwd/bwd).
    ``n`` (optional device int tensor: the rollout's early-exit width, e.g. from ``model.sample(..., {'async': True})`` or
    ``scst_rollouts(..., trim=False)``) lets the caller pass full-width (m, L) rollout outputs without ever syncing on n;
    ``reward`` may be (m, n'), one value per video (m, 1), one per position (1, L), a scalar, or 1-D of length m / L when
    m != L (m == L is ambiguous and raises)."""

    def forward(self, input, seq, reward, n=None):
        reward = torch.as_tensor(reward, dtype=torch.float32, device=input.device)
        return _RewardFunction.apply(input, seq, reward, n)


class _PerVideoRewardFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, slp, seq, score, base, baseline, n):
        from . import _native_scst_video as nsv
        B, S, L = slp.shape
        dev = slp.device
        slp_c = slp.detach().contiguous().float()
        seq = seq.detach().contiguous().long()
        score = score.detach().contiguous().float()
        base = None if base is None else base.detach().contiguous().float()
        nd = None if n is None else n.detach().reshape(-1)[:1].to(torch.int32)
        adv = torch.empty(B, S, dtype=torch.float32, device=dev)
        partial = torch.empty(B, 2, dtype=torch.float32, device=dev)
        sums = torch.empty(2, dtype=torch.float32, device=dev)
        nv.check(nsv.lib().xgsv_reward_fwd(_stream(), nv.ptr(slp_c), nv.ptr(seq), nv.ptr(score), nv.ptr(base), baseline, nv.ptr(nd),
                                           B, S, L, nv.ptr(adv), nv.ptr(partial), nv.ptr(sums)), "xgsv_reward_fwd")
        ctx.meta = (B, S, L, seq, adv, nd, sums)
        ctx.mark_non_differentiable(adv)
        return sums[0] / sums[1], adv

    @staticmethod
    def backward(ctx, dloss, dadv):
        from . import _native_scst_video as nsv
        B, S, L, seq, adv, nd, sums = ctx.meta
        dslp = torch.empty(B, S, L, dtype=torch.float32, device=sums.device)
        dl = dloss.detach().reshape(1).contiguous().float().to(sums.device)      # device scalar: no sync
        nv.check(nsv.lib().xgsv_reward_bwd(_stream(), nv.ptr(seq), nv.ptr(adv), nv.ptr(nd), B, S, L, nv.ptr(sums), nv.ptr(dl),
                                           nv.ptr(dslp)), "xgsv_reward_bwd")
        return dslp, None, None, None, None, None


class PerVideoRewardCriterion(nn.Module):
    """RewardCriterion over B videos x S rollouts with ONE score per row and the advantage formed on the device (include/
    xgate_scst_video.h): ``crit(seqLogprobs (B,S,L), seq (B,S,L), score (B,S), n=None, baseline="mean_others")`` returns
    -sum(seqLogprobs * adv * mask) / sum(mask), mask as in RewardCriterion (`n`: the rollout's device-side width).  baseline:
    "mean_others" (adv = score minus the mean of the video's other S - 1 scores; S >= 2), None (adv = score) or a (B,) tensor (adv =
    score - baseline[b]; S = 1 with the greedy rollout's score is the reference's self-critical reward).  ``last_advantage`` holds
    the (B,S) advantages of the last call.  The sums take no float atomics: two identical calls give identical bits."""

    def __init__(self):
        super().__init__()
        self.last_advantage = None

    def forward(self, input, seq, score, n=None, baseline="mean_others"):
        from ._native_scst_video import XGSV_BASE_GIVEN, XGSV_BASE_MEAN_OTHERS, XGSV_BASE_NONE
        if not torch.is_tensor(input) or input.dim() != 3:
            raise ValueError("seqLogprobs (B,S,L) expected")
        B, S, L = input.shape
        if not torch.is_tensor(seq) or tuple(seq.shape) != (B, S, L):
            raise ValueError("seq %s expected, got %s" % ((B, S, L), tuple(seq.shape) if torch.is_tensor(seq) else type(seq)))
        score = torch.as_tensor(score, dtype=torch.float32, device=input.device)
        if tuple(score.shape) != (B, S):
            raise ValueError("score %s expected, got %s" % ((B, S), tuple(score.shape)))
        base = None
        if baseline is None:
            mode = XGSV_BASE_NONE
        elif isinstance(baseline, str):
            if baseline != "mean_others":
                raise ValueError('baseline: "mean_others", None or a (B,) tensor expected, got %r' % (baseline,))
            if S < 2:
                raise ValueError('baseline "mean_others" needs S >= 2 rollouts per video, got %d' % S)
            mode = XGSV_BASE_MEAN_OTHERS
        else:
            base = torch.as_tensor(baseline, dtype=torch.float32, device=input.device)
            if tuple(base.shape) != (B,):
                raise ValueError("baseline (%d,) expected, got %s" % (B, tuple(base.shape)))
            mode = XGSV_BASE_GIVEN
        if not input.is_cuda or not seq.is_cuda:
            raise NotImplementedError("PerVideoRewardCriterion needs device tensors: there is no CPU path")
        loss, adv = _PerVideoRewardFunction.apply(input, seq, score, base, mode, n)
        self.last_advantage = adv
        return loss
