"""Host wrappers over the C ABI (include/pcy.h): weight packing, descriptors, KV cache, packing of
varlen protein batches.  torch is plumbing only -- device memory, streams, index arithmetic; all
model arithmetic runs in libpcy.so's HIP kernels.  No fallback path exists.
"""
from __future__ import annotations

import ctypes as C
import os
import math
from dataclasses import dataclass

import torch

from . import _lib as L

BF16 = torch.bfloat16


def _p(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _chk_bf16(*ts):
    for t in ts:
        if t is not None:
            assert t.is_cuda and t.dtype == BF16 and t.is_contiguous(), (t.dtype, t.device, t.is_contiguous())


class Context:
    """One engine context per (device, stream).  Launches go to torch's current stream."""
    _cache = {}

    def __init__(self, device=None):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise L.PcyError("no HIP device visible: the ProCyon engine needs an MI355X (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.device = dev
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
        h = C.c_void_p()
        L.check(self.lib.pcy_ctx_create(dev.index or 0, C.c_void_p(stream), C.byref(h)), "pcy_ctx_create")
        self.h = h

    @classmethod
    def get(cls, device=None):
        L.load()
        if not torch.cuda.is_available():
            raise L.PcyError("no HIP device visible: the ProCyon engine needs an MI355X (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        key = (dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)
        if key not in cls._cache:
            cls._cache[key] = Context(dev)
        return cls._cache[key]

    def sync(self):
        L.check(self.lib.pcy_ctx_sync(self.h), "sync")

    def timer_start(self):
        L.check(self.lib.pcy_timer_start(self.h), "timer_start")

    def timer_stop(self):
        ms = C.c_float()
        L.check(self.lib.pcy_timer_stop(self.h, C.byref(ms)), "timer_stop")
        return ms.value

    # ---- primitive ops -------------------------------------------------------------------------
    def gemm(self, A, W, bias=None, resid=None, epi=L.EPI_STORE, out=None):
        _chk_bf16(A, W, bias, resid)
        M, K = A.shape
        N = W.shape[0]
        Nout = N // 2 if epi == L.EPI_SWIGLU else N
        out = torch.empty(M, Nout, dtype=BF16, device=A.device) if out is None else out
        L.check(self.lib.pcy_gemm(self.h, _p(A), K, _p(W), _p(bias), _p(resid), 0 if resid is None else resid.shape[1],
                                  _p(out), Nout, M, N, K, epi), "pcy_gemm")
        return out

    def gemv(self, W, x, bias=None, resid=None, epi=L.EPI_STORE, rms_w=None, rms_eps=1e-5, rms_cast=0, out=None):
        _chk_bf16(W, x, bias, resid, rms_w)
        B, K = x.shape
        N = W.shape[0] // 2 if epi == L.EPI_SWIGLU else W.shape[0]
        out = torch.empty(B, N, dtype=BF16, device=x.device) if out is None else out
        L.check(self.lib.pcy_gemv(self.h, _p(W), _p(x), K, _p(bias), _p(resid), _p(out), N, _p(rms_w), rms_eps, rms_cast,
                                  N, K, B, epi), "pcy_gemv")
        return out

    def gemv_w8(self, W8, scale, x, resid=None, epi=L.EPI_STORE, rms_w=None, rms_eps=1e-5, rms_cast=0, out=None):
        """Weight-only fp8 GEMV (pcy_gemv_w8): epi((x . f32(W8)^T) * scale) -> bf16; W8 [N,K] uint8 (e4m3 bits) and scale [N] fp32 as
        `quant_rows_fp8` makes them, x [B,K] bf16 with 1 <= B <= 8; epi STORE / RESID / SWIGLU (W8 in the gate/up interleave)."""
        _chk_bf16(x, resid, rms_w)
        B, K = x.shape
        N = W8.shape[0] // 2 if epi == L.EPI_SWIGLU else W8.shape[0]
        out = torch.empty(B, N, dtype=BF16, device=x.device) if out is None else out
        L.check(self.lib.pcy_gemv_w8(self.h, _p(W8), _p(scale), _p(x), x.stride(0), _p(resid), _p(out), out.stride(0), _p(rms_w), rms_eps,
                                     rms_cast, N, K, B, epi), "pcy_gemv_w8")
        return out

    def lm_head_xent(self, x, W, targets, want_parts=False):
        """Teacher-forced scoring operator (pcy_lm_head_xent): per row m of x [M, d] (final-normed, bf16) against W [V, d] (lm_head),
        nll[m] = logsumexp(bf16 logits of the row) - bf16 logit of targets[m], HF's causal-LM loss term -- the [M, V] logits stay in
        registers.  -> nll [M] fp32, or with want_parts (nll, lse, row_max, label_logit), all [M] fp32."""
        _chk_bf16(x, W)
        M, d = x.shape
        V = W.shape[0]
        tg = targets.to(x.device, torch.int32).contiguous()
        assert tg.numel() == M, (tg.shape, M)
        nll = torch.empty(M, dtype=torch.float32, device=x.device)
        parts = [torch.empty_like(nll) for _ in range(3)] if want_parts else [None] * 3
        L.check(self.lib.pcy_lm_head_xent(self.h, _p(x), d, _p(W), M, V, d, _p(tg), _p(nll), *[_p(t) for t in parts]), "pcy_lm_head_xent")
        return (nll, *parts) if want_parts else nll

    def decode_mlp(self, x, ln2, wgu, wdown, rms_eps=1e-5, rms_cast=0):
        """One token through a Llama MLP, in place: x[1, d] += down(SwiGLU(gate/up(RMSNorm(x) * ln2))); wgu packed like gemv(EPI_SWIGLU)."""
        _chk_bf16(x, ln2, wgu, wdown)
        d, ffn = x.shape[-1], wdown.shape[1]
        L.check(self.lib.pcy_decode_mlp(self.h, _p(x), _p(ln2), _p(wgu), _p(wdown), d, ffn, rms_eps, rms_cast), "pcy_decode_mlp")
        return x

    def quant_rows_fp8(self, x):
        """Per-row symmetric OCP e4m3 quantisation of a bf16 matrix [rows,K] -> (q uint8 [rows,K], scale fp32 [rows])."""
        _chk_bf16(x)
        rows, K = x.shape
        q = torch.empty(rows, K, dtype=torch.uint8, device=x.device)
        sc = torch.empty(rows, dtype=torch.float32, device=x.device)
        L.check(self.lib.pcy_quant_rows_fp8(self.h, _p(x), x.stride(0), rows, K, _p(q), _p(sc)), "pcy_quant_rows_fp8")
        return q, sc

    def gemm_fp8(self, A8, sa, W8, sw, resid=None, epi=L.EPI_STORE, out=None):
        """epi(((A8 . W8^T) * sa[:,None]) * sw[None,:]) -> bf16; A8 [M,K], W8 [N,K] uint8 (e4m3 bits), sa [M], sw [N] fp32."""
        M, K = A8.shape
        N = W8.shape[0]
        Nout = N // 2 if epi == L.EPI_SWIGLU else N
        out = torch.empty(M, Nout, dtype=BF16, device=A8.device) if out is None else out
        L.check(self.lib.pcy_gemm_fp8(self.h, _p(A8), _p(sa), _p(W8), _p(sw), _p(resid), 0 if resid is None else resid.shape[1],
                                      _p(out), Nout, M, N, K, epi), "pcy_gemm_fp8")
        return out

    def rmsnorm(self, x, w, eps=1e-5, cast=0):
        _chk_bf16(x, w)
        y = torch.empty_like(x)
        L.check(self.lib.pcy_rmsnorm(self.h, _p(x), _p(w), _p(y), x.numel() // x.shape[-1], x.shape[-1], eps, cast), "rmsnorm")
        return y

    def layernorm(self, x, w, b, eps=1e-5):
        _chk_bf16(x, w, b)
        y = torch.empty_like(x)
        L.check(self.lib.pcy_layernorm(self.h, _p(x), _p(w), _p(b), _p(y), x.numel() // x.shape[-1], x.shape[-1], eps), "layernorm")
        return y

    def embed_splice(self, table, ids, soft=None, soft_map=None):
        """ids int32 [rows]; soft_map int32 [rows] (-1 = take table row)."""
        _chk_bf16(table, soft)
        rows, d = ids.numel(), table.shape[1]
        out = torch.empty(rows, d, dtype=BF16, device=table.device)
        L.check(self.lib.pcy_embed_splice(self.h, _p(table), _p(ids), _p(soft), _p(soft_map), _p(out), rows, d), "embed_splice")
        return out

    def rope_(self, buf, col0, nh, dh, pos, cos_t, sin_t, mode=0, prescale=0.0):
        """in place on a token-major [ntok, ld] buffer"""
        _chk_bf16(buf, cos_t, sin_t)
        L.check(self.lib.pcy_rope(self.h, _p(buf), buf.shape[1], col0, nh, dh, _p(pos), _p(cos_t), _p(sin_t), buf.shape[0],
                                  mode, prescale), "pcy_rope")
        return buf

    def attention(self, q, k, v, lens, H, Hkv, dh, causal, scale, keep=None, ld=None, col0=None):
        """q [ntok,H*dh], k,v [ntok,Hkv*dh] packed sequences of lengths `lens` (list).
        ld / col0: q, k, v as column windows of wider token-major buffers -- ld = the row stride in elements (one int for all three, or
        (ldq, ldk, ldv)), col0 = (qcol0, kcol0, vcol0), the column of head 0 in each.  The fused QKV buffer of the Llama prefill is
        q = k = v = buf [ntok, (H+2Hkv)*dh], ld = (H+2Hkv)*dh, col0 = (0, H*dh, (H+Hkv)*dh).  Default: the tensors' own width, column 0."""
        _chk_bf16(q, k, v)
        lds = (q.shape[1], k.shape[1], v.shape[1]) if ld is None else ((ld,) * 3 if isinstance(ld, int) else tuple(ld))
        c0 = (0, 0, 0) if col0 is None else tuple(col0)
        if ld is not None or col0 is not None:      # the kernels trust ld / col0: every window must lie inside its tensor
            for t, l_, c_, w in ((q, lds[0], c0[0], H * dh), (k, lds[1], c0[1], Hkv * dh), (v, lds[2], c0[2], Hkv * dh)):
                if not (t.is_contiguous() and c_ >= 0 and c_ + w <= l_ and t.numel() >= (sum(lens) - 1) * l_ + c_ + w):
                    raise ValueError("attention: column window outside its buffer")
        lens_t = torch.tensor(lens, dtype=torch.int64)
        cu = torch.zeros(len(lens) + 1, dtype=torch.int64)
        cu[1:] = lens_t.cumsum(0)
        vt_cu = torch.zeros(len(lens) + 1, dtype=torch.int64)
        vt_cu[1:] = ((lens_t + 31) // 32 * 32).cumsum(0)
        cu_d, vt_d = cu.to(q.device, torch.int32), vt_cu.to(q.device, torch.int32)
        o = torch.empty(q.shape[0], H * dh, dtype=BF16, device=q.device)
        L.check(self.lib.pcy_attention(self.h, _p(q), lds[0], c0[0], _p(k), lds[1], c0[1], _p(v), lds[2], c0[2], _p(o), H * dh,
                                       _p(cu_d), _p(vt_d), _p(keep), len(lens), int(lens_t.max()), int(vt_cu[-1]), H, Hkv, dh,
                                       int(causal), scale), "pcy_attention")
        return o

    def attn_decode(self, qkv, kcache, vcache, pos, cos_t, sin_t, H, Hkv, dh, keep=None, out=None):
        """qkv [B,(H+2Hkv)*dh]; kcache/vcache [B,Hkv,Tmax,dh]; pos int32 device scalar."""
        B, Tmax = kcache.shape[0], kcache.shape[2]
        o = torch.empty(B, H * dh, dtype=BF16, device=qkv.device) if out is None else out
        L.check(self.lib.pcy_attn_decode(self.h, _p(qkv), qkv.shape[1], _p(kcache), _p(vcache), _p(o), H * dh, _p(pos), _p(cos_t),
                                         _p(sin_t), _p(keep), B, H, Hkv, dh, Tmax), "pcy_attn_decode")
        return o

    def attn_decode_shared(self, qkv, cache, layer, pos, cos_t, sin_t, H, Hkv, dh, keep=None, B=None, out=None):
        """pcy_attn_decode_shared: `attn_decode`'s operator on layer `layer` of a shared-prefix KVCache, all rows of a prompt against one pass
        over its prefix.  qkv [B, (H+2Hkv)*dh] un-roped projections (B rows, default the cache's); pos int32 device scalar =
        the LOGICAL cache length; appends K / V at suffix slot pos - prefix_T; -> o [B, H*dh].  keep: [B, cache.capacity] uint8 in logical
        slots or None.  Anything but a complete shared-prefix cache with rows_per_prefix >= 1 is an error: there is no fallback."""
        _chk_bf16(qkv)
        B = cache.B if B is None else int(B)
        if keep is not None:
            assert keep.dtype == torch.uint8 and keep.is_contiguous() and tuple(keep.shape) == (B, cache.capacity), (keep.shape, keep.dtype)
        o = torch.empty(B, H * dh, dtype=BF16, device=qkv.device) if out is None else out
        L.check(self.lib.pcy_attn_decode_shared(self.h, _p(qkv), qkv.shape[1], C.byref(cache.c), int(layer), _p(o), o.shape[1], _p(pos), _p(cos_t),
                                                _p(sin_t), _p(keep), B, H, Hkv, dh), "pcy_attn_decode_shared")
        return o

    def attn_decode_split(self, qkv, cache, layer, pos, cos_t, sin_t, H, Hkv, dh, keep=None, B=None, out=None):
        """pcy_attn_decode_split: `attn_decode_shared`'s operator, arguments and errors on the split-key kernels: two launches,
        softmax statistics per key chunk (`attn_split_chunk_keys`) folded in a fixed-order combine.  Not the bits of `attn_decode_shared`."""
        _chk_bf16(qkv)
        B = cache.B if B is None else int(B)
        if keep is not None:
            assert keep.dtype == torch.uint8 and keep.is_contiguous() and tuple(keep.shape) == (B, cache.capacity), (keep.shape, keep.dtype)
        o = torch.empty(B, H * dh, dtype=BF16, device=qkv.device) if out is None else out
        L.check(self.lib.pcy_attn_decode_split(self.h, _p(qkv), qkv.shape[1], C.byref(cache.c), int(layer), _p(o), o.shape[1], _p(pos), _p(cos_t),
                                               _p(sin_t), _p(keep), B, H, Hkv, dh), "pcy_attn_decode_split")
        return o

    def attn_split_chunk_keys(self, B, rows_per_prefix, H, Hkv, dh, prefix_T):
        """keys per prefix chunk of `attn_decode_split`'s plan: host arithmetic on these six values only"""
        return int(self.lib.pcy_attn_split_chunk_keys(int(B), int(rows_per_prefix), int(H), int(Hkv), int(dh), int(prefix_T)))

    def attn_extend(self, qkv, cache, layer, t_past, cos_t, sin_t, H, Hkv, dh, keep=None, B=None, packed=False, groups=None):
        """pcy_attn_extend: qkv [B*S, (H+2Hkv)*dh] un-roped projections of S new tokens per row (row b*S+s; B rows, default the cache's);
        `cache` a KVCache (plain or shared-prefix) that holds t_past tokens per row.  Ropes q / k in place at t_past + s, appends K / V at
        logical slots t_past .. of layer `layer`, -> o [B*S, H*dh].  keep: [B, cache.capacity] uint8 in logical slots or None.
        packed: pcy_attn_extend_packed -- the queries of a prompt's rows and of a kv head's query heads share workgroups (same bits).
        groups: a grouped cache (`new_grouped_cache`) whose tables describe the rows -- pcy_attn_extend_grouped on `cache`; t_past then counts the
        tokens already in the rows' OWN panels (t_own)."""
        _chk_bf16(qkv)
        B = cache.B if B is None else int(B)
        S = qkv.shape[0] // B
        assert S * B == qkv.shape[0], (qkv.shape, B)
        if keep is not None:
            assert keep.dtype == torch.uint8 and keep.is_contiguous() and tuple(keep.shape) == (B, cache.capacity), (keep.shape, keep.dtype)
        o = torch.empty(B * S, H * dh, dtype=BF16, device=qkv.device)
        if groups is not None:
            ga = groups.groups_arg(t_past)
            L.check(self.lib.pcy_attn_extend_grouped(self.h, _p(qkv), qkv.shape[1], C.byref(cache.c), C.byref(ga), int(layer), _p(o), H * dh, _p(cos_t),
                                                     _p(sin_t), _p(keep), B, S, H, Hkv, dh, int(bool(packed))), "pcy_attn_extend_grouped")
            return o
        fn = self.lib.pcy_attn_extend_packed if packed else self.lib.pcy_attn_extend
        L.check(fn(self.h, _p(qkv), qkv.shape[1], C.byref(cache.c), int(layer), _p(o), H * dh, int(t_past), _p(cos_t), _p(sin_t), _p(keep),
                   B, S, H, Hkv, dh), "pcy_attn_extend")
        return o

    def attn_window(self, qkv, cache, layer, pos, cos_t, sin_t, H, Hkv, dh, out=None):
        """pcy_attn_window: qkv [W, (H+2Hkv)*dh] un-roped projections of W consecutive tokens of the ONE row of a plain KVCache;
        pos int32 device scalar = the slot of row 0, read on the device.  Ropes q / k of row i at pos + i (qkv itself is not written), writes
        K / V to slot pos + i of layer `layer`, -> o [W, H*dh], o[i] = the causal attention of query i over slots [0, pos + i].  2 <= W <= 32;
        a shared-prefix or grouped cache, or more than one cache row, is an error: there is no fallback."""
        _chk_bf16(qkv)
        W = qkv.shape[0]
        o = torch.empty(W, H * dh, dtype=BF16, device=qkv.device) if out is None else out
        L.check(self.lib.pcy_attn_window(self.h, _p(qkv), qkv.shape[1], C.byref(cache.c), int(layer), _p(o), o.shape[1], _p(pos), _p(cos_t),
                                         _p(sin_t), W, H, Hkv, dh), "pcy_attn_window")
        return o

    def attn_window_chunk(self):
        """keys per chunk of `attn_window` (a constant of the library)"""
        return int(self.lib.pcy_attn_window_chunk())

    def retrieval_scores(self, query, targets):
        """cosine similarities [Q,N] (bf16) as `ProcyonRetrievalEval.get_predictions` forms them (procyon.py:400-406)."""
        _chk_bf16(query, targets)
        Q, D = query.shape
        N = targets.shape[0]
        out = torch.empty(Q, N, dtype=BF16, device=query.device)
        L.check(self.lib.pcy_retrieval_scores(self.h, _p(query), Q, _p(targets), N, D, _p(out)), "pcy_retrieval_scores")
        return out

    def retrieval_topk(self, query, targets, k=None):
        """(indices int64 [Q,k], scores bf16 [Q,k]) of the k most similar targets per query, best first, ties by lower index
        (`get_proteins_from_embedding`, data/inference_utils.py:921-978); k=None ranks all N targets."""
        _chk_bf16(query, targets)
        Q, D = query.shape
        N = targets.shape[0]
        k = N if k is None else min(int(k), N)
        idx = torch.empty(Q, k, dtype=torch.int32, device=query.device)
        sc = torch.empty(Q, k, dtype=BF16, device=query.device)
        L.check(self.lib.pcy_retrieval_topk(self.h, _p(query), Q, _p(targets), N, D, k, _p(idx), _p(sc)), "pcy_retrieval_topk")
        return idx.long(), sc

    def qa_probs(self, logits, yes_id=None, no_id=None, want_probs=True, want_argmax=False):
        """The QA read-out on the device (pcy_qa_probs): `logits.softmax(dim=-1)` over the vocabulary for answer rows [rows, V] in the rows'
        dtype (bf16: fp32 statistics, one rounding; fp32), optionally the yes / no columns [rows, 2] (fp32 values of the stored
        probabilities) and the argmax of the stored probabilities -- data/inference_utils.py:582-604, training/train_utils.py:1048-1070.
        -> (probs | None, yes_no | None, argmax int64 | None)"""
        x = logits.to(self.device).contiguous()
        assert x.dim() == 2 and x.dtype in (BF16, torch.float32), (x.shape, x.dtype)
        rows, V = x.shape
        probs = torch.empty_like(x) if want_probs else None
        yn = torch.empty(rows, 2, dtype=torch.float32, device=x.device) if yes_id is not None else None
        am = torch.empty(rows, dtype=torch.int32, device=x.device) if want_argmax else None
        L.check(self.lib.pcy_qa_probs(self.h, _p(x), int(x.dtype == torch.float32), rows, V, int(yes_id or 0), int(no_id or 0), _p(probs), _p(yn),
                                      _p(am)), "pcy_qa_probs")
        return probs, yn, None if am is None else am.long()

    def _ret_f32_args(self, query, targets):
        q = query.to(self.device, torch.float32).contiguous()
        t = targets.to(self.device)
        if t.dtype != BF16:
            t = t.to(torch.float32)
        t = t.contiguous()
        assert q.dim() == 2 and t.dim() == 2 and q.shape[1] == t.shape[1], (q.shape, t.shape)
        return q, t, int(t.dtype == BF16)

    def retrieval_scores_f32(self, query, targets):
        """fp32 cosine similarities [Q,N] (fp32 accumulation, fp32 result); query any float dtype, targets fp32 or bf16 -- the
        scoring of `get_proteins_from_batched_embeddings` (data/inference_utils.py:981-999)."""
        q, t, tb = self._ret_f32_args(query, targets)
        out = torch.empty(q.shape[0], t.shape[0], dtype=torch.float32, device=self.device)
        L.check(self.lib.pcy_retrieval_scores_f32(self.h, _p(q), q.shape[0], _p(t), tb, t.shape[0], q.shape[1], _p(out)), "pcy_retrieval_scores_f32")
        return out

    def retrieval_topk_f32(self, query, targets, k=None):
        """(indices int64 [Q,k], scores fp32 [Q,k]) ranked on fp32 similarities, best first, ties by lower index
        (`get_proteins_from_embedding`, data/inference_utils.py:921-978); k=None ranks all N targets."""
        q, t, tb = self._ret_f32_args(query, targets)
        N = t.shape[0]
        k = N if k is None else min(int(k), N)
        idx = torch.empty(q.shape[0], k, dtype=torch.int32, device=self.device)
        sc = torch.empty(q.shape[0], k, dtype=torch.float32, device=self.device)
        L.check(self.lib.pcy_retrieval_topk_f32(self.h, _p(q), q.shape[0], _p(t), tb, N, q.shape[1], k, _p(idx), _p(sc)), "pcy_retrieval_topk_f32")
        return idx.long(), sc

    def pool(self, hidden, seg, rng, nprot, mode):
        _chk_bf16(hidden)
        d = hidden.shape[-1]
        out = torch.empty(nprot, d, dtype=BF16, device=hidden.device)
        L.check(self.lib.pcy_pool(self.h, _p(hidden), d, _p(seg), _p(rng), nprot, mode, _p(out)), "pool")
        return out


# ------------------------------------------------------------------------------------------------
class MlpEngine:
    """`create_mlp` projector (reference procyon/model/model_utils.py:13-41), eval mode."""

    def __init__(self, layers, ctx=None):
        self.ctx = ctx or Context.get()
        self.layers = [(w.contiguous(), None if b is None else b.contiguous()) for w, b in layers]
        n = len(self.layers)
        assert 1 <= n <= 8
        d = L.MlpDesc()
        d.n_layers = n
        d.dims[0] = self.layers[0][0].shape[1]
        for i, (w, b) in enumerate(self.layers):
            _chk_bf16(w, b)
            d.dims[i + 1] = w.shape[0]
            d.w[i] = w.data_ptr()
            d.b[i] = 0 if b is None else b.data_ptr()
        self.desc = d
        self.in_features, self.out_features = d.dims[0], d.dims[n]
        self.src_f32 = None      # fp32 (W, b) pairs of the same projector, set by the loader when the checkpoint is fp32
        self._f32 = None

    def f32(self):
        """the same projector in fp32 arithmetic (procyon_amd.engine_f32), for a model that was never cast to bf16"""
        if self._f32 is None:
            if self.src_f32 is None:
                raise RuntimeError("fp32 arithmetic was asked for, but this projector holds no fp32 weights")
            from .engine_f32 import MlpEngineF32
            self._f32 = MlpEngineF32(self.src_f32, self.ctx)
        return self._f32

    def drop_fp32(self):
        self.src_f32 = self._f32 = None

    def __call__(self, x):
        if x.dtype == torch.float32:
            return self.f32()(x)
        shape = x.shape
        x = x.reshape(-1, shape[-1]).contiguous()
        _chk_bf16(x)
        out = torch.empty(x.shape[0], self.out_features, dtype=BF16, device=x.device)
        if x.shape[0]:
            L.check(self.ctx.lib.pcy_mlp_forward(self.ctx.h, C.byref(self.desc), _p(x), x.shape[0], _p(out)), "pcy_mlp_forward")
        return out.reshape(*shape[:-1], self.out_features)


# ------------------------------------------------------------------------------------------------
def rope_tables(dh, theta, n_pos, device, inv_freq_bf16=False):
    """cos/sin [n_pos, dh] bf16.  Default: fp32 inv_freq, table rounded once (transformers 4.31's cached
    tables).  inv_freq_bf16=True reproduces transformers 5.x after `.bfloat16()`."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.float32) / dh))
    if inv_freq_bf16:
        inv_freq = inv_freq.to(BF16).float()
    pos = torch.arange(n_pos, dtype=torch.float32)
    freqs = (inv_freq[:, None] @ pos[None, :]).transpose(0, 1)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(BF16).to(device).contiguous(), emb.sin().to(BF16).to(device).contiguous()


@dataclass
class LlamaConfig:
    vocab: int
    d: int
    n_layers: int
    n_heads: int
    n_kv_heads: int
    ffn: int
    rms_eps: float = 1e-5
    rope_theta: float = 10000.0   # reference-compat default (App. B Q9); Llama-3's own value is 500000
    max_pos: int = 8192
    rms_cast: str = "hf5"         # 'hf5' (>=4.32) or 'hf431'
    rope_inv_freq_bf16: bool = False

    @property
    def head_dim(self):
        return self.d // self.n_heads


def interleave_gate_up(gate, up):
    """[F,d],[F,d] -> [2F,d] with 16-row gate/up interleave (layout the SwiGLU epilogues expect)."""
    F_, d = gate.shape
    assert F_ % 16 == 0
    return torch.stack([gate.view(F_ // 16, 16, d), up.view(F_ // 16, 16, d)], dim=1).reshape(2 * F_, d).contiguous()


class _Stager:
    """Host -> device upload of the small int32 index arrays of one engine call without stalling the stream and without a
    pinned allocation per call: a ring of persistent pinned staging buffers (grown on demand), ONE async copy per call into
    one device buffer, views handed out (a pageable source would make the copy wait for the queued GPU work, and the
    retrieval loop would alternate host packing and GPU encoding instead of overlapping them).  Measured equal to a
    `pin_memory()` copy per array (tools/archive/t_esm_percall.py: 22.1 ms per call at batch 8, 56.4 ms at batch 25, back to back);
    it replaces six pinned allocations and copies per call by one."""
    SLOTS = 3

    def __init__(self, device):
        self.device = torch.device(device)
        self.slots = [None] * self.SLOTS
        self.events = [None] * self.SLOTS
        self.i = 0

    def upload(self, arrays, into=None):
        """arrays: CPU int32 tensors -> list of device int32 tensors (views of one device buffer, 256-byte aligned).
        `into`: a persistent device uint8 buffer to copy into instead of a fresh one (same sizes -> the views keep their addresses
        from call to call: what a replayed launch chain needs)."""
        offs, total = [], 0
        for a in arrays:
            offs.append(total)
            total += (a.numel() * 4 + 255) // 256 * 256
        total = max(total, 256)
        k = self.i % len(self.slots)
        if self.events[k] is not None and not self.events[k].query():
            # the copy from this slot is still queued behind earlier kernels: never wait for the stream here (the host would
            # serialise with the GPU); take a fresh slot instead -- the ring grows to the number of calls in flight
            self.slots.insert(k, None)
            self.events.insert(k, None)
        if self.slots[k] is None or self.slots[k].numel() < total:
            self.slots[k] = torch.empty(max(total, 1 << 20) * 2, dtype=torch.uint8).pin_memory()
        host = self.slots[k]
        for a, o in zip(arrays, offs):
            n = a.numel() * 4
            host[o:o + n].view(torch.int32).copy_(a.contiguous().view(-1))
        devbuf = torch.empty(total, dtype=torch.uint8, device=self.device) if into is None else into[:total]
        devbuf.copy_(host[:total], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.events[k] = ev
        self.i = k + 1
        return [devbuf[o:o + a.numel() * 4].view(torch.int32).view(a.shape) for a, o in zip(arrays, offs)]


_stagers = {}


def _h2d_many(arrays, dev, into=None):
    dev = torch.device(dev)
    if dev.type != "cuda":
        return [a.to(dev) for a in arrays]
    if into is None and os.environ.get("PCY_STAGER", "1") == "0":      # A/B: a pinned copy per array and call (the previous behaviour)
        outs = []
        for a in arrays:
            src = a.contiguous().pin_memory()
            o = src.to(dev, non_blocking=True)
            o._pcy_src = src
            outs.append(o)
        return outs
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _stagers:
        _stagers[key] = _Stager(dev)
    return _stagers[key].upload(arrays, into)


class KVCache:
    """[L,B,Hkv,Tmax,dh] x2; `layer(l)` gives the reference's past_key_values[l] views.

    With `prefix` (a B'-row prefill cache whose Tmax is the prompt length T, see LlamaEngine.new_beam_cache) the B rows share its K / V:
    row b reads prefix row b // rows_per_prefix for logical slots [0, T) and owns only the suffix slots [T, T + Tmax) held in k / v
    (include/pcy.h, pcy_kv_cache).  `Tmax` is then the suffix capacity and `capacity` the logical one."""

    def __init__(self, cfg: LlamaConfig, B, Tmax, device, prefix: "KVCache" = None, rows_per_prefix=0):
        self.k = torch.zeros(cfg.n_layers, B, cfg.n_kv_heads, Tmax, cfg.head_dim, dtype=BF16, device=device)
        self.v = torch.zeros_like(self.k)
        self.B, self.Tmax = B, Tmax
        self.prefix, self.rows_per_prefix = prefix, int(rows_per_prefix)
        if prefix is None:
            self.c = L.KvCache(self.k.data_ptr(), self.v.data_ptr(), B, Tmax)
        else:
            if prefix.prefix is not None or self.rows_per_prefix < 1 or B > prefix.B * self.rows_per_prefix:
                raise ValueError(f"shared-prefix cache: {B} rows of {rows_per_prefix} per prefix row on a {prefix.B}-row plain prefix cache")
            self.c = L.KvCache(self.k.data_ptr(), self.v.data_ptr(), B, Tmax, prefix.k.data_ptr(), prefix.v.data_ptr(), prefix.B, prefix.Tmax,
                               self.rows_per_prefix)

    @property
    def prefix_T(self):
        return 0 if self.prefix is None else self.prefix.Tmax

    @property
    def capacity(self):
        """logical key slots per row: what the position counter and the keep mask count in"""
        return self.prefix_T + self.Tmax

    @classmethod
    def grouped(cls, cfg, device, prefix: "KVCache", group_rows, group_len, suffix_slots):
        """A cache whose rows are GROUPS over the rows of `prefix` (LlamaEngine.new_grouped_cache; include/pcy.h, pcy_prefix_groups): group g
        = group_rows[g] contiguous rows that read the first group_len[g] slots of prefix row g, their own panels right behind.  Holds the host
        lists and the device tables of the call argument; `c.rows_per_prefix` is 0, which every entry but the grouped ones refuses."""
        rows, lens = [int(r) for r in group_rows], [int(n) for n in group_len]
        if prefix is None or prefix.prefix is not None:
            raise ValueError("grouped cache: the prefix must be a plain cache")
        if not rows or len(rows) != len(lens):
            raise ValueError(f"grouped cache: {len(rows)} group_rows for {len(lens)} group_len (at least one group each)")
        if len(rows) > prefix.B:
            raise ValueError(f"grouped cache: {len(rows)} groups on a prefix cache of {prefix.B} rows")
        if min(rows) < 1:
            raise ValueError(f"grouped cache: group_rows {rows}: every group holds at least one row")
        if min(lens) < 1 or max(lens) > prefix.Tmax:
            raise ValueError(f"grouped cache: group_len {lens} outside [1, {prefix.Tmax}]")
        if int(suffix_slots) < 1:
            raise ValueError(f"grouped cache: suffix_slots={suffix_slots}")
        self = cls.__new__(cls)
        B = sum(rows)
        self.k = torch.zeros(cfg.n_layers, B, cfg.n_kv_heads, int(suffix_slots), cfg.head_dim, dtype=BF16, device=device)
        self.v = torch.zeros_like(self.k)
        self.B, self.Tmax, self.prefix, self.rows_per_prefix = B, int(suffix_slots), prefix, 0
        self.group_rows, self.group_len = rows, lens
        self.c = L.KvCache(self.k.data_ptr(), self.v.data_ptr(), B, self.Tmax, prefix.k.data_ptr(), prefix.v.data_ptr(), prefix.B, prefix.Tmax, 0)
        row0 = [0]
        for r in rows:
            row0.append(row0[-1] + r)
        self.row_group = [g for g, r in enumerate(rows) for _ in range(r)]
        i32 = lambda x: torch.tensor(x, dtype=torch.int32)
        self.d_row0, self.d_len, self.d_row_grp = _h2d_many([i32(row0), i32(lens), i32(self.row_group)], torch.device(device))
        self._h_rows, self._h_len = (C.c_int32 * len(rows))(*rows), (C.c_int32 * len(lens))(*lens)
        return self

    def groups_arg(self, t_own):
        """the pcy_prefix_groups of a call with t_own tokens already in the rows' own panels (the tables live as long as the cache)"""
        return L.PrefixGroups(len(self.group_rows), int(t_own), self._h_rows, self._h_len, self.d_row0.data_ptr(), self.d_len.data_ptr(),
                              self.d_row_grp.data_ptr())

    @property
    def is_grouped(self):
        return getattr(self, "group_rows", None) is not None

    def row_len(self):
        """[B] prefix length of every row of a grouped cache"""
        return torch.tensor([self.group_len[g] for g in self.row_group])

    def layer(self, l, t):
        if self.prefix is None:
            return self.k[l, :, :, :t], self.v[l, :, :, :t]
        if self.is_grouped:
            # (tests / debugging only) per row: its group's real prefix slots, then t of its own -> lists of [Hkv, len + t, dh]
            ks = [torch.cat([self.prefix.k[l, g, :, :self.group_len[g]], self.k[l, b, :, :t]], 1) for b, g in enumerate(self.row_group)]
            vs = [torch.cat([self.prefix.v[l, g, :, :self.group_len[g]], self.v[l, b, :, :t]], 1) for b, g in enumerate(self.row_group)]
            return ks, vs
        # (tests / debugging only: the logical [B, Hkv, t, dh] rows materialised, prefix rows repeated + suffix)
        Tp = self.prefix_T
        rows = torch.arange(self.B, device=self.k.device) // self.rows_per_prefix
        pk, pv = self.prefix.k[l][rows, :, :min(t, Tp)], self.prefix.v[l][rows, :, :min(t, Tp)]
        if t <= Tp:
            return pk, pv
        return torch.cat([pk, self.k[l, :, :, :t - Tp]], 2), torch.cat([pv, self.v[l, :, :, :t - Tp]], 2)


def uniform_keep(prefix_mask, suffix_mask, Tp):
    """keep [R, Tp + S] int64 of an extension on a `new_shared_cache`: the prefixes' mask [P, Tp] (None: ones), every row of it repeated for
    the R // P rows behind that prefix, then the rows' own suffix_mask [R, S]"""
    R = suffix_mask.shape[0]
    head = torch.ones(R, Tp, dtype=torch.long) if prefix_mask is None else prefix_mask.repeat_interleave(R // prefix_mask.shape[0], 0)
    return torch.cat([head, suffix_mask], 1)


def grouped_keep(row_len, Tp, suffix_mask):
    """keep [R, Tp + S] int64 of an extension on a `new_grouped_cache`, in every row's OWN logical slots: ones on its row_len[r] prefix slots,
    its suffix_mask [R, S] right behind them, zeros from there on"""
    S = suffix_mask.shape[1]
    col = torch.arange(Tp + S)[None] - row_len[:, None]                      # the column counted from the row's first own slot
    own = suffix_mask.long().gather(1, col.clamp(0, S - 1)) * ((col >= 0) & (col < S))
    return own + (col < 0)


# The beams of a prompt share ONE copy of its K / V (KVCache with a prefix) when the plan below says so.  A pure function of the call's shape
# and the PCY_DISABLE names: the rule lives here and nowhere else.
#   beam > 1                     -- one row per prompt has nothing to share
#   B * beam > BEAM_SHARED_MIN_ROWS_ABOVE (8 = the upper clamp of PCY_NB_MAX) -- the small-batch one-launch step serves up to that many rows and
#                                   reads plain caches only: it is never displaced, whatever the switches say
#   none of beam_kv_shared / beam_prefill_once / beam_kv_suffix in PCY_DISABLE -- the shared cache IS "prefill once" and "reorder the suffix
#                                   only"; with either twin asked for, the plain cache serves it
BEAM_SHARED_MIN_ROWS_ABOVE = 8


def beam_cache_plan(B, beam, T, max_new, disabled_names=()):
    """-> dict(shared, rows, prefix_rows, prefix_slots, suffix_slots, slots_shared, slots_plain): whether a beam search of B prompts x beam
    beams over T prompt tokens and max_new generated ones runs on a shared-prefix cache, and the K (= V) slots per layer and kv head of
    the two layouts: B*T + B*beam*max_new against B*beam*(T + max_new)."""
    B, beam, T, max_new = int(B), int(beam), int(T), int(max_new)
    off = set(disabled_names)
    rows = B * beam
    shared = beam > 1 and rows > BEAM_SHARED_MIN_ROWS_ABOVE and not (off & {"beam_kv_shared", "beam_prefill_once", "beam_kv_suffix"})
    return dict(shared=bool(shared), rows=rows, prefix_rows=B, prefix_slots=T, suffix_slots=max_new,
                slots_shared=B * T + rows * max_new, slots_plain=rows * (T + max_new))


# The decode step for more than 32 rows (LlamaEngine.decode_gemm): from how many rows `decode_gemm="auto"` takes it.  The default
# step streams the weights once per 32 rows, the new one once per step: DECODE_GEMM_MIN_ROWS is the smallest measured row count from which the
# new step won every pair of tools/bench_decode_gemm.py on both geometries (profiles/decode_gemm_ab.log).  Never below 33.
DECODE_GEMM_MIN_ROWS = 33


def decode_gemm_plan(rows, shared=False, mha=False):
    """-> bool: whether `decode_gemm="auto"` runs a decode step of `rows` rows on the one-pass GEMM step.  shared: the cache carries a shared
    prefix; mha: the multi-head geometry class (Llama-2-7B / ProCyon-Split) instead of the grouped-query one (Llama-3-8B).  Pure: the one
    place that decides what "auto" means.  The measurement gave the same threshold for both classes and both cache layouts."""
    return int(rows) >= max(33, DECODE_GEMM_MIN_ROWS)


def check_shared_attn(shared_attn):
    """-> False, True or "split": the values of the `shared_attn` option, anything else a ValueError.  False: the per-row decode attention;
    True: the many-queries attention of the GEMM step; "split": the split-key attention, beam search only."""
    if shared_attn is False or shared_attn is True:
        return shared_attn
    if isinstance(shared_attn, str) and shared_attn == "split":
        return "split"
    raise ValueError(f"shared_attn={shared_attn!r}: False, True or 'split'")


def disabled_switches():
    """The names in PCY_DISABLE (procyon_amd/csrc/pcy_switch.h: comma separated, whole names), read now: the one reader on the Python side."""
    return frozenset(n.strip() for n in os.environ.get("PCY_DISABLE", "").split(",") if n.strip())


STOP_CHUNK = 8      # decode steps enqueued between two looks at `done`: steps_until_done's and beam_steps_until_done's number


class EosStop:
    """The EOS stop of a generation state (the trailing fields of pcy_gen_state), shared by GenState and
    engine_f32.GenStateF32.  eos_id=None: no stop -- nothing is allocated and the four fields of the C struct stay zero.  Otherwise
    `finished` [B], `done` and `n_steps_run` (device int32 scalars), all zero-initialised, and a pinned host row that takes one copy of
    `done` per chunk of steps."""

    def _init_stop(self, B, eos_id, device, max_steps):
        self.eos_id = None if eos_id is None else int(eos_id)
        self.finished = self.done = self.n_steps_run = self._done_host = None
        self._n_looks = 0
        if eos_id is not None:
            self.finished = torch.zeros(B, dtype=torch.int32, device=device)
            self.done = torch.zeros(1, dtype=torch.int32, device=device)
            self.n_steps_run = torch.zeros(1, dtype=torch.int32, device=device)
            self._done_host = torch.zeros(max_steps // STOP_CHUNK + 3, dtype=torch.int32, pin_memory=True)

    def _stop_args(self):
        if self.eos_id is None:
            return (None, None, None, 0)
        return (self.finished.data_ptr(), self.done.data_ptr(), self.n_steps_run.data_ptr(), self.eos_id)

    @property
    def steps_run(self):
        """rows of tokens_out / of the logits record that a pick has written (reads *step back: synchronises).  Without a stop, or when no
        launch raised `done`: every step that was enqueued.  With a stop: the step of the last row's EOS + 1, exactly -- the picks behind
        `done` change nothing, *step included."""
        return int(self.step)

    def look_at_done(self):
        """an asynchronous copy of `done` to the host behind what the stream holds now -> a callable that waits for THAT copy only (not for
        what is enqueued after it) and returns the flag"""
        slot = self._done_host[self._n_looks % self._done_host.numel():][:1]
        self._n_looks += 1
        slot.copy_(self.done, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()

        def flag():
            ev.synchronize()
            return bool(int(slot))
        return flag


def steps_until_done(st, total, enqueue, first_look=None):
    """`total` decode steps of a state with an EOS stop, enqueued by `enqueue(n)` in chunks of STOP_CHUNK, until a look at `done` says that
    every row has emitted its EOS.  The look at the chunk before is read while the latest chunk runs: one chunk at most is in flight ahead
    of the read, and the stream never drains.  Worst case: the flag raised by the first step of a chunk is read after the next chunk was
    enqueued -- 2 * STOP_CHUNK - 1 = 15 decode steps behind the finishing one, each followed by a pick that changes nothing.  first_look: the
    look behind whatever the caller ran in front (the pick on the prefill's logits).  Returns the steps enqueued."""
    pending, i = first_look, 0
    while i < total:
        n = min(STOP_CHUNK, total - i)
        enqueue(n)
        i += n
        look = st.look_at_done()
        if pending is not None and pending():
            break
        pending = look
    return i


def finish_stop(st, la):
    """What a driver with an EOS stop hands out, behind a synchronisation: (tokens [B, max_steps] int64 with eos_id in every slot behind a
    row's EOS -- the steps never run included --, the logits record cut to [B, steps_run, V])"""
    n = st.steps_run
    tok = st.tokens_out.long()
    tok[:, n:] = st.eos_id
    return tok, (None if la is None else la[:, :n])


def hand_out(st):
    """What a greedy, sampling or lookahead driver returns from a state that is ALREADY synchronised: (tokens [B, max_steps] int64,
    logprob [B], the logits record [B, steps_run, V] | None) -- with an EOS stop `finish_stop`'s tokens and record, without one every slot."""
    la = None if st.logits_all is None else st.logits_all.transpose(0, 1)
    tok, la = (st.tokens_out.long(), la) if st.eos_id is None else finish_stop(st, la)
    return tok, st.logprob, la


def run_generation(st, max_len, first_pick, enqueue, sync):
    """The loop behind a prefill of every greedy and sampling driver: `first_pick()` on the prefill's logits; the max_len - 1 steps, by
    `enqueue(n)` = n x (decode step + pick) without a host synchronisation, at once or under the state's EOS stop in chunks; `sync()` (the
    record may live in host memory, and a watchdog that fired inside a fused launch must fail THIS call); then `hand_out`."""
    first_pick()
    if max_len > 1 and st.eos_id is None:
        enqueue(max_len - 1)
    elif max_len > 1:
        steps_until_done(st, max_len - 1, enqueue, st.look_at_done())
    sync()
    return hand_out(st)


def sampling_variates(uniforms, max_len, B, device):
    """The variates uniforms[step * B + b] of a sampling call, float32 and contiguous on `device`: ONE `torch.rand` of max_len * B, or the
    caller's `uniforms` -- more are accepted, fewer are a ValueError (the picks would read beyond the allocation)."""
    n = int(max_len) * int(B)
    if uniforms is None:
        return torch.rand(n, device=device, dtype=torch.float32)
    if uniforms.numel() < n:
        raise ValueError(f"generate_sampling: {uniforms.numel()} uniform variates for {max_len} steps x {B} rows: {n} are needed")
    return uniforms.to(device, torch.float32).contiguous()


def beam_parent_index(anc):
    """anc [steps, BB]: the parent slot of every slot at every step -> idx [steps, BB] int64, the slot that held at step s what slot r holds
    after the last step (the record of step s is re-indexed by the parents of every step >= s).  Pure."""
    steps, BB = anc.shape
    anc = anc.long()
    slot = torch.arange(BB, device=anc.device)
    idx = torch.empty(steps, BB, dtype=torch.long, device=anc.device)
    for s in range(steps - 1, -1, -1):
        slot = anc[s][slot]
        idx[s] = slot
    return idx


def beam_hand_out(bs, rec, max_len, sync):
    """What a device-side beam search returns from its state and its per-slot record rec [max_len, BB, V]: (tokens [BB, max_len] int64, zeros
    behind an early EOS stop, and scores [BB] on the host, logits [BB, steps, V] along the parent chain: gathered on the device, then ONE copy
    into pinned host memory -- a pageable destination moves a beam-10 record at a few GB/s, ~1 ms per generated token).  sync() comes last."""
    out, steps = bs.tokens()                                   # synchronises
    idx = beam_parent_index(bs.anc[:steps])
    BB, V = rec.shape[1:]
    rec_dev = rec[:steps].gather(1, idx[:, :, None].expand(steps, BB, V)).transpose(0, 1).contiguous()
    out_logits = torch.empty(rec_dev.shape, dtype=rec.dtype, pin_memory=True)
    out_logits.copy_(rec_dev, non_blocking=True)
    tokens, scores = torch.nn.functional.pad(out.cpu(), (0, max_len - steps)), bs.cur.cpu()
    sync()
    return tokens, scores, out_logits


def beam_steps_until_done(bs, max_len, advance):
    """Steps 1 .. max_len - 1 of a beam search: `advance(i, n_max)` enqueues 1..n_max steps from step i and returns how many; n_max never
    crosses the next multiple of STOP_CHUNK or max_len, and `bs.done` is read (a synchronisation) only where i is such a multiple."""
    i = 1
    while i < max_len and not (i % STOP_CHUNK == 0 and int(bs.done)):
        i += advance(i, min(STOP_CHUNK - i % STOP_CHUNK, max_len - i))
    return i


def check_stop_arg(stop_on_eos, vocab, what):
    """What a driver's `stop_on_eos=None | eos_id` means: None, or the id as an int inside the vocabulary (ValueError otherwise)"""
    if stop_on_eos is None:
        return None
    if isinstance(stop_on_eos, bool) or not isinstance(stop_on_eos, int) or not 0 <= stop_on_eos < vocab:
        raise ValueError(f"{what}: stop_on_eos={stop_on_eos!r}: None or a token id in [0, {vocab})")
    return stop_on_eos


class GenState(EosStop):
    def __init__(self, B, vocab, max_steps, device, keep_logits=False, keep=None, pos=None, next_tok=None, eos_id=None):   # pos, next_tok: see BeamState.gen_state
        self.pos = torch.zeros(1, dtype=torch.int32, device=device) if pos is None else pos
        self.step = torch.zeros(1, dtype=torch.int32, device=device)
        self.next_tok = torch.zeros(B, dtype=torch.int32, device=device) if next_tok is None else next_tok
        self.tokens_out = torch.zeros(B, max_steps, dtype=torch.int32, device=device)
        self.logprob = torch.zeros(B, dtype=torch.float32, device=device)
        self.logits = torch.empty(B, vocab, dtype=BF16, device=device)
        # the per-step logits record is what the reference returns on the CPU: pinned host memory written by the decode steps
        # themselves (rows padded to a multiple of 8 elements for 16-byte stores); PCY_LOGITS_HOST=0 keeps it on the device
        self.logits_all = self._logits_host = None
        ld = vocab
        if keep_logits:
            if os.environ.get("PCY_LOGITS_HOST", "1") != "0":
                ld = (vocab + 7) // 8 * 8
                self._logits_host = torch.empty(max_steps, B, ld, dtype=BF16, pin_memory=True)
                self.logits_all = self._logits_host[:, :, :vocab]
            else:
                self.logits_all = torch.empty(max_steps, B, vocab, dtype=BF16, device=device)
        self.keep = keep
        self._init_stop(B, eos_id, device, max_steps)
        self.c = L.GenState(self.pos.data_ptr(), self.step.data_ptr(), self.next_tok.data_ptr(), self.tokens_out.data_ptr(),
                            self.logprob.data_ptr(), self.logits.data_ptr(),
                            0 if self.logits_all is None else self.logits_all.data_ptr(),
                            0 if keep is None else keep.data_ptr(), max_steps, ld, *self._stop_args())


class BeamState:
    """Device-side state of the diverse beam search (pcy_beam_step): token histories (double-buffered), running scores,
    parent slots per step, EOS flags, step / position / done scalars."""

    def __init__(self, B, beam, max_len, eos_id, prompt_len, device):
        BB = B * beam
        z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=device)
        self.B, self.beam, self.BB, self.max_len = B, beam, BB, max_len
        self.out = z(2, BB, max_len)
        self.cur, self.cur_new = z(BB, dtype=torch.float32), z(BB, dtype=torch.float32)
        self.next_tok, self.src, self.anc = z(BB), z(BB), z(max_len, BB)
        self.has_eos = z(2, BB, dtype=torch.uint8)
        self.blk_eos, self.ticket = z(B), z(1)
        self.pos = torch.full((1,), prompt_len, dtype=torch.int32, device=device)
        self.step, self.done = z(1), z(1)
        self.c = L.BeamState(self.out.data_ptr(), max_len, self.cur.data_ptr(), self.cur_new.data_ptr(), self.next_tok.data_ptr(),
                             self.src.data_ptr(), self.anc.data_ptr(), self.has_eos.data_ptr(), self.blk_eos.data_ptr(),
                             self.ticket.data_ptr(), self.pos.data_ptr(), self.step.data_ptr(), self.done.data_ptr(), int(eos_id))

    def gen_state(self, vocab):
        """The decode state of the BB rows on this state's own position and next-token arrays: the decode step reads what the beam step writes."""
        return GenState(self.BB, vocab, 1, self.pos.device, pos=self.pos, next_tok=self.next_tok)

    def tokens(self):
        """[BB, steps] int64 histories after the steps run so far (syncs)."""
        steps = int(self.step)
        return self.out[steps & 1, :, :steps].long(), steps


def lookup_draft(hist, window, ngram_max, ngram_min):
    """The draft rule of greedy decoding with lookahead (include/pcy.h, pcy_look_state; the device twin is pcy_look_draft) in plain Python:
    hist = the prompt's token ids followed by every committed token (negative = no text token) -> the window - 1 drafts.  For g = ngram_max
    down to ngram_min: the LARGEST i with i + g < n and hist[i:i+g] == hist[n-g:n], every compared entry >= 0; the drafts are what followed,
    hist[i+g], hist[i+g+1], ... until the history ends or an entry is negative; whatever is not filled that way is the filler hist[n-1]."""
    h = [int(t) for t in hist]
    n, W = len(h), int(window)
    if n < 1 or W < 2:
        raise ValueError(f"lookup_draft: a history of {n} tokens, window {W}")
    drafts = []
    for g in range(int(ngram_max), int(ngram_min) - 1, -1):
        if g < 1 or g >= n or min(h[n - g:]) < 0:
            continue
        hit = next((i for i in range(n - g - 1, -1, -1) if h[i:i + g] == h[n - g:]), None)
        if hit is not None:
            for t in h[hit + g:hit + g + W - 1]:
                if t < 0:
                    break
                drafts.append(t)
            break
    return drafts + [h[n - 1]] * (W - 1 - len(drafts))


def lookahead_passes(tokens, prompt_ids, window, ngram=(3, 1), forced=None):
    """How many passes `LlamaEngine.generate_lookahead` takes for a KNOWN greedy token sequence `tokens` (token 0 comes from the prefill):
    -> (passes, accepted histogram [window]: passes that committed k drafts).  Each pass drafts by `lookup_draft` over prompt_ids + the tokens
    committed so far (forced[i] >= 0 replaces the draft of output token i), accepts the leading drafts that equal the sequence and commits one
    token more, clamped at the end of the sequence."""
    toks, W = [int(t) for t in tokens], int(window)
    hist = [int(t) for t in prompt_ids] + toks[:1]
    step, passes, accepted = 1, 0, [0] * W
    while step < len(toks):
        drafts = lookup_draft(hist, W, ngram[0], ngram[1])
        if forced is not None:
            drafts = [int(forced[step + j]) if step + j < len(forced) and int(forced[step + j]) >= 0 else t for j, t in enumerate(drafts)]
        a = 0
        while a < W - 1 and step + a < len(toks) and drafts[a] == toks[step + a]:
            a += 1
        n = min(a + 1, len(toks) - step)
        hist += toks[step:step + n]
        step += n
        passes += 1
        accepted[n - 1] += 1
    return passes, accepted


class LookState:
    """Device-side state of greedy decoding with lookahead for one prompt (include/pcy.h, pcy_look_state), beside a one-row GenState."""

    def __init__(self, hist_ids, max_new, window, ngram, device, forced=None):
        T = int(hist_ids.numel())
        self.W, self.cap = int(window), T + int(max_new)
        self.hist = torch.full((self.cap,), -1, dtype=torch.int32, device=device)
        self.hist[:T] = hist_ids.to(device, torch.int32).view(-1)
        self.n_hist = torch.full((1,), T, dtype=torch.int32, device=device)
        self.window = torch.zeros(self.W, dtype=torch.int32, device=device)
        self.counters = torch.zeros(2 + self.W, dtype=torch.int32, device=device)
        self.last = torch.zeros(4, dtype=torch.int32, device=device)
        self.forced = None if forced is None else forced.to(device, torch.int32).contiguous()
        self.c = L.LookState(self.hist.data_ptr(), self.n_hist.data_ptr(), self.window.data_ptr(),
                             0 if self.forced is None else self.forced.data_ptr(), self.counters.data_ptr(), self.last.data_ptr(),
                             self.cap, self.W, int(ngram[0]), int(ngram[1]))

    def stats(self):
        """-> dict(passes, tokens (committed by passes: the prefill's token 0 is not one), accepted [W] (passes that committed k drafts),
        tokens_per_pass)"""
        c = self.counters.cpu().tolist()
        return dict(passes=c[0], tokens=c[1], accepted=c[2:], tokens_per_pass=(c[1] / c[0] if c[0] else 0.0))


def score_plan(full_labels, T_real, vocab):
    """Which token rows a teacher-forced scoring pass scores, and against what -- HF's shift (`logits[:, :-1]` against `labels[:, 1:]`,
    ignore_index -100), on the host, no device involved.  full_labels [B, T] (-100 = not scored); the engine runs T_real columns, so row
    (b, t) is scored against full_labels[b, t + 1] for t + 1 < T_real wherever that label is not -100.
    -> (score_rows int32 [n] = b * T_real + t, targets int32 [n], index int64 [n, 2] of the (b, t) pairs), row-major.
    A label outside [0, vocab) other than -100 raises ValueError."""
    lab = torch.as_tensor(full_labels).detach().cpu().long()
    assert lab.dim() == 2, lab.shape
    T_real = int(T_real)
    nxt = lab[:, 1:T_real]
    scored = nxt != -100
    if bool((scored & ((nxt < 0) | (nxt >= int(vocab)))).any()):
        bad = nxt[scored & ((nxt < 0) | (nxt >= int(vocab)))]
        raise ValueError(f"full_labels hold {int(bad[0])}: labels must lie in [0, {int(vocab)}) or be -100")
    bt = scored.nonzero()
    rows = (bt[:, 0] * T_real + bt[:, 1]).to(torch.int32)
    return rows, nxt[scored].to(torch.int32), bt


class LlamaEngine:
    """HF-Llama-architecture decoder behind `LlamaPostTokenization.forward` (pmc_llama.py:546-596)."""

    def __init__(self, sd, cfg: LlamaConfig, device=None, ctx=None, free_source=False, fp8_prefill=False):
        """fp8_prefill: additionally keep per-output-channel e4m3 copies of the four projections of every layer and run
        the prefill's projections on the fp8 MFMA path (BASELINE configs[4]; `set_fp8(False)` switches back to bf16)."""
        self.ctx = ctx or Context.get(device)
        self.cfg = cfg
        dev = self.ctx.device
        self.device = dev
        g = lambda k: sd[k].to(dev, BF16).contiguous()
        self.embed = g("model.embed_tokens.weight")
        self.final_norm = g("model.norm.weight")
        self.lm_head = g("lm_head.weight")
        self.cos, self.sin = rope_tables(cfg.head_dim, cfg.rope_theta, cfg.max_pos, dev, cfg.rope_inv_freq_bf16)
        self._keep = []
        arr = (L.LlamaLayer * cfg.n_layers)()
        for l in range(cfg.n_layers):
            p = f"model.layers.{l}."
            wqkv = torch.cat([g(p + "self_attn.q_proj.weight"), g(p + "self_attn.k_proj.weight"),
                              g(p + "self_attn.v_proj.weight")], 0).contiguous()
            wo = g(p + "self_attn.o_proj.weight")
            wgu = interleave_gate_up(g(p + "mlp.gate_proj.weight"), g(p + "mlp.up_proj.weight"))
            wdown = g(p + "mlp.down_proj.weight")
            ln1, ln2 = g(p + "input_layernorm.weight"), g(p + "post_attention_layernorm.weight")
            self._keep.append((wqkv, wo, wgu, wdown, ln1, ln2))
            arr[l] = L.LlamaLayer(*[t.data_ptr() for t in (wqkv, wo, wgu, wdown, ln1, ln2)])
            if free_source:
                for k in [k for k in sd if k.startswith(p)]:
                    del sd[k]
        self._arr = arr
        self.desc = L.LlamaDesc(cfg.vocab, cfg.d, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.ffn,
                                cfg.max_pos, cfg.rms_eps, 0 if cfg.rms_cast == "hf5" else 1, self.embed.data_ptr(),
                                self.final_norm.data_ptr(), self.lm_head.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr(),
                                C.cast(arr, C.POINTER(L.LlamaLayer)))
        self._arr8 = None
        if fp8_prefill:
            self.quantize_fp8()

    def quantize_fp8(self):
        """e4m3 copies + per-row scales of wqkv / wo / wgu / wdown (8 GB on top of the 16 GB of a Llama-3-8B), fp8 path on."""
        self._ensure_fp8_copies()
        self.set_fp8(True)

    def _ensure_fp8_copies(self):
        """the e4m3 copies + per-row scales, built once; `desc.layers_fp8` (the prefill's switch) is not touched"""
        if self._arr8 is None:
            self._keep8 = []
            arr8 = (L.LlamaLayerFp8 * self.cfg.n_layers)()
            for l, ws in enumerate(self._keep):
                qs = [self.ctx.quant_rows_fp8(w) for w in ws[:4]]
                self._keep8.append(qs)
                arr8[l] = L.LlamaLayerFp8(*[q.data_ptr() for q, _ in qs], *[sc.data_ptr() for _, sc in qs])
            self._arr8 = arr8
        return self._arr8

    def set_fp8(self, on):
        if on and self._arr8 is None:
            raise ValueError("no fp8 weights: construct with fp8_prefill=True or call quantize_fp8()")
        self.desc.layers_fp8 = C.cast(self._arr8, C.POINTER(L.LlamaLayerFp8)) if on else C.POINTER(L.LlamaLayerFp8)()

    def new_cache(self, B, Tmax):
        return KVCache(self.cfg, B, Tmax, self.device)

    def new_shared_cache(self, prefix_cache: KVCache, rows_per_prefix, suffix_slots):
        """A cache of prefix_cache.B * rows_per_prefix rows that share the K / V of the prompts prefilled into `prefix_cache` (Tmax == the prompt
        length) and own `suffix_slots` slots each: what `extend` and the beam search run on.  Row r belongs to prompt r // rows_per_prefix."""
        n = int(rows_per_prefix)
        return KVCache(self.cfg, prefix_cache.B * n, int(suffix_slots), self.device, prefix=prefix_cache, rows_per_prefix=n)

    new_beam_cache = new_shared_cache   # (prefix_cache, beam, max_new): the same call in the beam search's words

    def new_grouped_cache(self, prefix_cache: KVCache, group_rows, group_len, suffix_slots):
        """A cache of sum(group_rows) rows in groups: group g = group_rows[g] contiguous rows that share the first group_len[g] slots of row g of
        `prefix_cache` (RIGHT-padded prompts: the real tokens start at position 0) and own `suffix_slots` slots each, right behind their prefix.
        What `extend(cache, embeds, own_past=...)` runs on; ValueError for tables the library would refuse."""
        return KVCache.grouped(self.cfg, self.device, prefix_cache, group_rows, group_len, suffix_slots)

    def embed_tokens(self, ids, soft=None, soft_map=None):
        """ids [B,T] int -> [B,T,d]; soft-token splice of `_prepare_input_embeddings` if soft_map given."""
        B, T = ids.shape
        i32 = ids.to(self.device, torch.int32).contiguous().view(-1)
        sm = None if soft_map is None else soft_map.to(self.device, torch.int32).contiguous().view(-1)
        return self.ctx.embed_splice(self.embed, i32, soft, sm).view(B, T, self.cfg.d)

    def _logit_rows(self, spec, B, T, allow_all):
        """the flat token rows b*T+t (int32, on the device) a call returns logits for"""
        dev = self.device
        if isinstance(spec, str):
            if spec == "last":
                return (torch.arange(B, dtype=torch.int32, device=dev) + 1) * T - 1
            if spec == "all" and allow_all:
                return torch.arange(B * T, dtype=torch.int32, device=dev)
            raise ValueError(f"logit_rows={spec!r}: expected " + ('"all", ' if allow_all else "") + '"last", None or a tensor of flat rows b*T+t')
        if spec is None:
            return torch.zeros(0, dtype=torch.int32, device=dev)
        return spec.to(dev, torch.int32).contiguous()

    def _score_upload(self, labels, B, T):
        """score_plan of `labels` on the device -> (n, score rows, targets, (b, t) pairs, nll [n] to fill: all None when n == 0; token_nll [B,T] = 0)"""
        rows_c, tg_c, bt = score_plan(labels, T, self.cfg.vocab)
        n, dev = int(rows_c.numel()), self.device
        up = (*_h2d_many([rows_c, tg_c, bt.to(torch.int32)], dev), torch.empty(n, dtype=torch.float32, device=dev)) if n else (None,) * 4
        return (n, *up, torch.zeros(B, T, dtype=torch.float32, device=dev))

    @staticmethod
    def _scatter_nll(token_nll, bt_d, nll):
        if nll is not None:   # row (b, t) scores the token at t + 1
            token_nll[bt_d[:, 0].long(), bt_d[:, 1].long() + 1] = nll

    def _prefill_args(self, embeds, attn_mask, logit_rows, all_rows=False):
        """What both prefill entry points hand the library -> (embeds contiguous, keep mask uint8 [B,T] | None when nothing is masked, positions,
        cu / vt_cu offsets, flat logit rows int32, logits [n,V] to fill).  logit_rows: "last", None, flat rows b*T+t; with all_rows also "all"."""
        B, T, _ = embeds.shape
        embeds = embeds.contiguous()
        _chk_bf16(embeds)
        dev = self.device
        keep = None
        if attn_mask is not None and not bool((attn_mask != 0).all()):
            keep = (attn_mask != 0).to(dev, torch.uint8).contiguous()
        pos = torch.arange(T, dtype=torch.int32, device=dev).repeat(B)
        cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * T
        vt_cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * ((T + 31) // 32 * 32)
        rows = self._logit_rows(logit_rows, B, T, all_rows)
        return embeds, keep, pos, cu, vt_cu, rows, torch.empty(rows.numel(), self.cfg.vocab, dtype=BF16, device=dev)

    def prefill(self, embeds, attn_mask, cache: KVCache, logit_rows="last", want_hidden=False, sum_rows=None):
        """embeds [B,T,d] bf16; attn_mask [B,T] (0/1) or None.  Returns (logits [n,V], hidden [B,T,d]|None), and with
        `sum_rows` (flat token rows b*T+t) additionally the sum over all L+1 hidden states of those rows [n,d]
        (ret_token_access='all')."""
        B, T, d = embeds.shape
        dev = self.device
        embeds, keep, pos, cu, vt_cu, rows, logits = self._prefill_args(embeds, attn_mask, logit_rows)
        hidden = torch.empty(B, T, d, dtype=BF16, device=dev) if want_hidden else None
        srows = None if sum_rows is None else sum_rows.to(dev, torch.int32).contiguous()
        ns = 0 if srows is None else srows.numel()
        hsum = torch.empty(ns, d, dtype=BF16, device=dev) if ns else None
        L.check(self.ctx.lib.pcy_llama_prefill(self.ctx.h, C.byref(self.desc), C.byref(cache.c), _p(embeds), _p(keep), _p(pos),
                                               _p(cu), _p(vt_cu), B, T, _p(rows), rows.numel(), _p(logits), _p(hidden), _p(srows), ns, _p(hsum)),
                "pcy_llama_prefill")
        if sum_rows is not None:
            return logits, hidden, hsum
        return logits, hidden

    def prefill_all(self, embeds, attn_mask, cache: KVCache, logit_rows="all"):
        """The prefill with everything `LlamaPostTokenization.forward` returns (pmc_llama.py:575-596): (logits [n,V] for
        `logit_rows` ("all" = every token row, the reference's [B,T,V]; "last"; None; or flat rows), hidden_states [L+1,B,T,d] =
        embeddings, outputs of layers 0..L-2, final-normed output of layer L-1)."""
        B, T, d = embeds.shape
        dev = self.device
        embeds, keep, pos, cu, vt_cu, rows, logits = self._prefill_args(embeds, attn_mask, logit_rows, all_rows=True)
        hidden_all = torch.empty(self.cfg.n_layers + 1, B, T, d, dtype=BF16, device=dev)
        L.check(self.ctx.lib.pcy_llama_prefill_all(self.ctx.h, C.byref(self.desc), C.byref(cache.c), _p(embeds), _p(keep), _p(pos),
                                                   _p(cu), _p(vt_cu), B, T, _p(rows), rows.numel(), _p(logits), _p(hidden_all)),
                "pcy_llama_prefill_all")
        return logits, hidden_all

    def score(self, embeds, attn_mask, full_labels, cache=None, logit_rows=None):
        """Teacher-forced scoring in ONE prefill pass (pcy_llama_score): embeds [B,T,d] bf16, attn_mask [B,T] or None, full_labels [B,>=T]
        (HF's `labels`: -100 = not scored; columns beyond T are not run).  -> (token_nll [B,T] fp32, n_tokens, logits | None):
        token_nll[b, t+1] = -log p(token t+1 | tokens <= t) where full_labels[b, t+1] is a label, 0 elsewhere; n_tokens = number of scored
        tokens; logits [n,V] for `logit_rows` (flat rows b*T+t or "last"; the bits of `prefill`) or None.  The [rows, V] logits of the scored
        rows are never materialised.  K/V go to `cache` (a scratch one when None).  Nothing is launched when there is nothing to do."""
        B, T, _ = embeds.shape
        n, srows, tg, bt_d, nll, token_nll = self._score_upload(full_labels, B, T)
        if n == 0 and logit_rows is None:
            return token_nll, 0, None
        cache = self.new_cache(B, T) if cache is None else cache
        embeds, keep, pos, cu, vt_cu, rows, logits = self._prefill_args(embeds, attn_mask, logit_rows)
        L.check(self.ctx.lib.pcy_llama_score(self.ctx.h, C.byref(self.desc), C.byref(cache.c), _p(embeds), _p(keep), _p(pos), _p(cu), _p(vt_cu),
                                             B, T, _p(srows), _p(tg), n, _p(nll), _p(rows), rows.numel(), _p(logits)), "pcy_llama_score")
        self._scatter_nll(token_nll, bt_d, nll)
        return token_nll, n, (logits if logit_rows is not None else None)

    def extend(self, cache: KVCache, embeds, t_past=None, keep=None, logit_rows=None, labels=None, want_hidden=False, packed=False, own_past=None):
        """S more tokens per row against a cache that holds t_past tokens per row (the library's extension, `_extend_call`; HF's forward(inputs_embeds [B,S],
        past_key_values)).  embeds [B,S,d] bf16; cache plain or shared-prefix (`new_shared_cache`); keep [B, >= t_past + S] (0 = masked key,
        old and new slots alike) or None; logit_rows "all" / "last" / flat rows b*S+s / None; labels [B,S] in HF's convention (-100 = not
        scored): token_nll[b, s+1] = -log p(token s+1 | everything up to s, the cached prefix included), 0 elsewhere.
        -> (logits [n,V] | None, hidden [B,S,d] | None, token_nll [B,S] fp32 | None, n_tokens).  K / V of slots [t_past, t_past+S) are written.
        packed: the packed entry -- the attention packs the queries of a prompt's rows into shared workgroups (same bits; it pays when
        many rows per prefix carry few new tokens each).
        A grouped cache (`new_grouped_cache`) takes `own_past` (default 0) instead of t_past: the tokens already in the rows' own panels; row b
        of group g then holds group_len[g] + own_past tokens, and keep [B, >= max over the rows of that + S] is in the row's own logical slots
        (the grouped entry)."""
        B, S, d = embeds.shape
        dev = self.device
        embeds = embeds.contiguous()
        _chk_bf16(embeds)
        grouped = cache.is_grouped
        if grouped:
            if t_past is not None:
                raise ValueError("extend: a grouped cache takes own_past (the tokens in the rows' own panels), not t_past")
            own_past = 0 if own_past is None else int(own_past)
            if B != cache.B:
                raise ValueError(f"extend: {B} rows on a grouped cache of {cache.B}")
            row_end = cache.row_len() + own_past + S                             # [B] keys of every row after the append
            t_past = int(row_end.max()) - S
        else:
            if own_past is not None:
                raise ValueError("extend: own_past belongs to a grouped cache (new_grouped_cache); this cache takes t_past")
            if t_past is None:
                raise ValueError("extend: t_past missing")
            row_end = None
        t_past = int(t_past)
        keep_d = None
        if keep is not None:
            kp = (torch.as_tensor(keep) != 0)
            if kp.dim() != 2 or kp.shape[0] != B or kp.shape[1] < min(t_past + S, cache.capacity):
                raise ValueError(f"keep {tuple(kp.shape)}: expected [{B}, >= {t_past + S}]")
            live = kp[:, :t_past + S] if row_end is None else (kp[:, :t_past + S] | (torch.arange(t_past + S)[None] >= row_end[:, None]))
            if not bool(live.all()):
                keep_d = torch.zeros(B, cache.capacity, dtype=torch.uint8, device=dev)   # (row stride = the logical capacity)
                n = min(kp.shape[1], cache.capacity)
                keep_d[:, :n] = kp[:, :n].to(dev, torch.uint8)
        rows = self._logit_rows(logit_rows, B, S, True)
        logits = torch.empty(rows.numel(), self.cfg.vocab, dtype=BF16, device=dev)
        hidden = torch.empty(B, S, d, dtype=BF16, device=dev) if want_hidden else None
        n, srows, tg, bt_d, nll, token_nll = self._score_upload(labels, B, S) if labels is not None else (0,) + (None,) * 5
        self._extend_call(cache, embeds, keep_d, own_past if grouped else t_past, packed, rows, logits, hidden, srows, tg, n, nll)
        self._scatter_nll(token_nll, bt_d, nll)
        return (logits if logit_rows is not None else None), hidden, token_nll, n

    def _extend_call(self, cache, embeds, keep_d, t_past, packed, rows, logits, hidden=None, srows=None, tg=None, n=0, nll=None):
        """The one call site of pcy_llama_extend / _packed / _grouped, on device tensors the caller has prepared (embeds [B,S,d], keep_d uint8
        [B, cache.capacity] | None, rows int32, logits [rows, V], ...); t_past of a grouped cache counts the tokens in the rows' own panels."""
        lib, (B, S, _) = self.ctx.lib, embeds.shape
        head = (self.ctx.h, C.byref(self.desc), C.byref(cache.c))
        tail = (_p(rows), rows.numel(), _p(logits), _p(hidden), _p(srows), _p(tg), n, _p(nll))
        if cache.is_grouped:
            ga = cache.groups_arg(t_past)
            L.check(lib.pcy_llama_extend_grouped(*head, C.byref(ga), _p(embeds), _p(keep_d), B, S, int(bool(packed)), *tail), "pcy_llama_extend_grouped")
        else:
            fn = lib.pcy_llama_extend_packed if packed else lib.pcy_llama_extend
            L.check(fn(*head, _p(embeds), _p(keep_d), B, S, int(t_past), *tail), "pcy_llama_extend")

    def extend_behind(self, prefix_emb, prefix_mask, suffix_emb, suffix_mask, rows_per_prefix=None, groups=None, **what):
        """Prefill P prefixes ONCE and run the rows behind them as ONE `extend`: prefix_emb [P,Tp,d]; suffix_emb [R,S,d], suffix_mask [R,S] (0 on
        the right pads).  Either rows_per_prefix (R = P * rows_per_prefix rows on a `new_shared_cache`; prefix_mask [P,Tp] with the pads on the
        LEFT, or None = no pads) or groups = (group_rows, group_len) (a `new_grouped_cache`; the prefixes RIGHT-padded to Tp, so group_len is
        their mask).  what: logit_rows / labels / want_hidden / packed of `extend`.  -> (*what `extend` returns, the cache).
        The key mask of the extension is None -- the kernels' unmasked block path -- whenever nothing is masked: no prefix pads and full suffixes."""
        P, Tp, _ = prefix_emb.shape
        S, full = suffix_emb.shape[1], bool(suffix_mask.all())
        prefix_cache = self.new_cache(P, Tp)
        if groups is not None:
            prefix_mask = (torch.arange(Tp)[None] < torch.tensor(groups[1])[:, None]).long()
        self.prefill(prefix_emb, prefix_mask, prefix_cache, logit_rows=None)
        if groups is not None:
            cache, t_past = self.new_grouped_cache(prefix_cache, *groups, S), None
            keep = None if full else grouped_keep(cache.row_len(), Tp, suffix_mask)
        else:
            cache, t_past = self.new_shared_cache(prefix_cache, rows_per_prefix, S), Tp
            keep = None if full and prefix_mask is None else uniform_keep(prefix_mask, suffix_mask, Tp)
        return (*self.extend(cache, suffix_emb, t_past, keep=keep, **what), cache)

    def extend_ws_bytes(self, B, S, n_logit_rows=0, n_score=0):
        """workspace of an `extend` call: host arithmetic, a function of the row counts only (never of the past length)"""
        return int(self.ctx.lib.pcy_llama_extend_ws_bytes(C.byref(self.desc), int(B), int(S), int(n_logit_rows), int(n_score)))

    def decode(self, cache: KVCache, st: GenState, B):
        L.check(self.ctx.lib.pcy_llama_decode(self.ctx.h, C.byref(self.desc), C.byref(cache.c), C.byref(st.c), B), "pcy_llama_decode")

    def decode_layers(self, cache: KVCache, st: GenState, B, reps=1):
        """measurement aid: `reps` passes over the decoder layers of a decode step (no embedding, no lm_head, no pick)."""
        L.check(self.ctx.lib.pcy_llama_decode_layers(self.ctx.h, C.byref(self.desc), C.byref(cache.c), C.byref(st.c), B, reps), "pcy_llama_decode_layers")

    def decode_graph(self, cache: KVCache, st: GenState, B):
        """decode step as one replayed hipGraph (~190 launches otherwise): loops that select between steps on the device."""
        L.check(self.ctx.lib.pcy_llama_decode_graph(self.ctx.h, C.byref(self.desc), C.byref(cache.c), C.byref(st.c), B), "pcy_llama_decode_graph")

    def decode_gemm(self, cache: KVCache, st: GenState, B, shared_attn=False):
        """the decode step for more than 32 rows: every projection one GEMM over the B rows, one pass over the weights (pcy_llama_decode_gemm).
        The contract of `decode`; not its bits.  shared_attn=True (pcy_llama_decode_gemm_mq): the attention scores all rows of a
        prompt against one pass over its shared prefix -- a shared-prefix cache only, anything else is an error.  shared_attn="split"
        (pcy_llama_decode_gemm_split): the same on the split-key attention's two launches."""
        if check_shared_attn(shared_attn) == "split":
            L.check(self.ctx.lib.pcy_llama_decode_gemm_split(self.ctx.h, C.byref(self.desc), C.byref(cache.c), C.byref(st.c), B), "pcy_llama_decode_gemm_split")
            return
        if shared_attn:
            L.check(self.ctx.lib.pcy_llama_decode_gemm_mq(self.ctx.h, C.byref(self.desc), C.byref(cache.c), C.byref(st.c), B), "pcy_llama_decode_gemm_mq")
            return
        L.check(self.ctx.lib.pcy_llama_decode_gemm(self.ctx.h, C.byref(self.desc), C.byref(cache.c), C.byref(st.c), B), "pcy_llama_decode_gemm")

    def decode_split(self, cache: KVCache, st: GenState, B):
        """`decode` on the default batched loop with every layer's attention served by the split-key launches (pcy_llama_decode_split, DESIGN.md
        4.3f): a shared-prefix cache with rows_per_prefix >= 1 and a row count the batched loop serves; anything else is an error.  The
        contract of `decode`; not its bits."""
        L.check(self.ctx.lib.pcy_llama_decode_split(self.ctx.h, C.byref(self.desc), C.byref(cache.c), C.byref(st.c), B), "pcy_llama_decode_split")

    def decode_w8(self, cache: KVCache, st: GenState, B):
        """the decode step that streams the e4m3 copies of the projections (pcy_llama_decode_w8): weight-only fp8, 1..8 rows,
        plain caches.  The contract of `decode`; not its bits.  The copies are made on first use; the prefill stays what `set_fp8` says."""
        L.check(self.ctx.lib.pcy_llama_decode_w8(self.ctx.h, C.byref(self.desc), self._ensure_fp8_copies(), C.byref(cache.c), C.byref(st.c), B),
                "pcy_llama_decode_w8")

    def greedy_steps_w8(self, cache, st, B, n_steps, use_graph=True):
        """n_steps x (decode_w8 + pick) with no host synchronisation; use_graph: one replayed hipGraph per step (pcy_llama_greedy_w8)"""
        L.check(self.ctx.lib.pcy_llama_greedy_w8(self.ctx.h, C.byref(self.desc), self._ensure_fp8_copies(), C.byref(cache.c), C.byref(st.c), B,
                                                 n_steps, int(use_graph)), "pcy_llama_greedy_w8")

    @staticmethod
    def _use_decode_w8(decode_w8, rows, decode_gemm=False):
        """What a driver's `decode_w8=False | True` means; ValueError for what the e4m3 step does not serve."""
        if decode_w8 is False:
            return False
        if decode_w8 is not True:
            raise ValueError(f"decode_w8={decode_w8!r}: False or True")
        if not (decode_gemm is False or decode_gemm is None):
            raise ValueError("decode_w8 and decode_gemm are two different decode steps: choose one")
        if rows > 8:
            raise ValueError(f"decode_w8 serves 1..8 rows, not {rows}")
        return True

    def _use_decode_gemm(self, decode_gemm, rows, shared=False):
        """What a driver's `decode_gemm=False | True | "auto"` means for `rows` decode rows."""
        if decode_gemm is False or decode_gemm is None:
            return False
        if decode_gemm is True:
            return True
        if decode_gemm == "auto":
            return decode_gemm_plan(rows, shared, self.cfg.n_kv_heads == self.cfg.n_heads)
        raise ValueError(f"decode_gemm={decode_gemm!r}: False, True or 'auto'")

    def beam_step(self, logits, bs: "BeamState", group_size, diversity_penalty):
        """one step of the reference's diverse-beam bookkeeping on the device (pcy_beam_step); logits [BB, vocab] bf16."""
        _chk_bf16(logits)
        L.check(self.ctx.lib.pcy_beam_step(self.ctx.h, _p(logits), logits.shape[1], bs.B, bs.beam, group_size, float(diversity_penalty),
                                           C.byref(bs.c)), "pcy_beam_step")

    def beam_steps(self, cache: KVCache, st: GenState, bs: "BeamState", group_size, diversity_penalty, logits_rec, n_steps, kv_t0=0, split=False):
        """n_steps iterations of decode -> record -> beam step -> KV reorder, each ONE replayed launch chain
        (pcy_llama_beam_steps); st.pos / st.next_tok are the beam state's arrays.  kv_t0: first cache slot the reorder moves (the prompt
        length when the beams of a prompt hold the same prefix rows).  split: the chain's decode step is `decode_split`'s
        (pcy_llama_beam_steps_split)."""
        name = "pcy_llama_beam_steps_split" if split else "pcy_llama_beam_steps"
        L.check(getattr(self.ctx.lib, name)(self.ctx.h, C.byref(self.desc), C.byref(cache.c), C.byref(st.c), bs.B, bs.beam, group_size,
                                            float(diversity_penalty), C.byref(bs.c), _p(logits_rec), n_steps, int(kv_t0)), name)

    def pick(self, cache: KVCache, st: GenState, B, advance_pos):
        L.check(self.ctx.lib.pcy_greedy_pick(self.ctx.h, C.byref(self.desc), C.byref(cache.c), C.byref(st.c), B, int(advance_pos)),
                "pcy_greedy_pick")

    def greedy_steps(self, cache, st, B, n_steps, use_graph=True):
        L.check(self.ctx.lib.pcy_llama_greedy(self.ctx.h, C.byref(self.desc), C.byref(cache.c), C.byref(st.c), B, n_steps,
                                              int(use_graph)), "pcy_llama_greedy")

    def sample_pick(self, cache, st, B, advance_pos, uniforms, temperature=1.0, nucleus_prob=None, probs_out=None):
        """sampling / nucleus selection on st.logits with the uniform variates uniforms[step * B + b] (pcy_sample_pick)"""
        L.check(self.ctx.lib.pcy_sample_pick(self.ctx.h, C.byref(self.desc), C.byref(cache.c), C.byref(st.c), B, int(advance_pos),
                                             float(temperature), -1.0 if nucleus_prob is None else float(nucleus_prob), _p(uniforms), _p(probs_out)),
                "pcy_sample_pick")

    def sample_steps(self, cache, st, B, n_steps, uniforms, temperature=1.0, nucleus_prob=None):
        L.check(self.ctx.lib.pcy_llama_sample(self.ctx.h, C.byref(self.desc), C.byref(cache.c), C.byref(st.c), B, n_steps, float(temperature),
                                              -1.0 if nucleus_prob is None else float(nucleus_prob), _p(uniforms)), "pcy_llama_sample")

    def _prefill_for_generation(self, embeds, attn_mask, max_len, keep_logits, keep=None, eos_id=None, spare_slots=0):
        """How greedy, sampling and lookahead open: a cache of T + max_len (+ spare_slots) slots, the state, the prompts prefilled, their
        last-row logits in st.logits, pos = T."""
        B, T, _ = embeds.shape
        cache = self.new_cache(B, T + max_len + spare_slots)
        st = GenState(B, self.cfg.vocab, max_len, self.device, keep_logits, keep, eos_id=eos_id)
        logits, _ = self.prefill(embeds, attn_mask, cache, "last")
        st.logits.copy_(logits)
        st.pos.fill_(T)
        return cache, st

    def generate_sampling(self, embeds, attn_mask, max_len, temperature=1.0, nucleus_prob=None, keep_logits=False, uniforms=None, decode_gemm=False,
                          decode_w8=False, stop_on_eos=None):
        """`_generate_sampling(greedy=False)` (model_unified.py:861-921) entirely on the device: prefill, then per step the
        decode launches + the sampling kernels (pcy_llama_sample); the uniform variates of all steps are drawn up front from
        torch's device generator (one `torch.rand`) unless `uniforms` [>= max_len * B] injects them (`sampling_variates`: fewer are a ValueError
        before the prefill).  Returns (tokens [B,max_len] int64, logprob [B], logits | None, state).
        decode_gemm (False | True | "auto"): the steps on the one-pass GEMM step, one decode_gemm + sample_pick per step.
        decode_w8 (False | True): the steps on the e4m3 weight stream, one decode_w8 + sample_pick per step.
        stop_on_eos (None | eos_id): as in `generate_greedy` -- the sampling pick raises `done`, the variates keep their positions
        uniforms[step * B + b], so a row's draws are those of the call without a stop."""
        B = embeds.shape[0]
        w8 = self._use_decode_w8(decode_w8, B, decode_gemm)
        gemm = self._use_decode_gemm(decode_gemm, B)
        eos = check_stop_arg(stop_on_eos, self.cfg.vocab, "generate_sampling")
        u = sampling_variates(uniforms, max_len, B, self.device)
        cache, st = self._prefill_for_generation(embeds, attn_mask, max_len, keep_logits, eos_id=eos)
        if gemm or w8:
            step = self.decode_w8 if w8 else self.decode_gemm

            def run(n):      # no host synchronisation inside: the step reads the token and the position from the device
                for _ in range(n):
                    step(cache, st, B)
                    self.sample_pick(cache, st, B, True, u, temperature, nucleus_prob)
        else:
            run = lambda n: self.sample_steps(cache, st, B, n, u, temperature, nucleus_prob)
        first = lambda: self.sample_pick(cache, st, B, False, u, temperature, nucleus_prob)
        return run_generation(st, max_len, first, run, self.ctx.sync) + ((st, cache, u),)

    def kv_reorder(self, cache, src_rows, t, t0=0):
        """cache[:, b] = cache[:, src_rows[b]] over slots [t0, t) (t0 > 0: the rows are known to hold the same contents below t0)"""
        src = src_rows.to(self.device, torch.int32).contiguous()
        L.check(self.ctx.lib.pcy_kv_reorder_range(self.ctx.h, C.byref(self.desc), C.byref(cache.c), _p(src), src.numel(), int(t0), t), "pcy_kv_reorder")

    def generate_greedy(self, embeds, attn_mask, max_len, keep_logits=False, clean_decode_mask=False, use_graph=True, decode_gemm=False,
                        decode_w8=False, stop_on_eos=None):
        """`_generate_sampling(greedy=True)` (model_unified.py:861-921): prefill, then max_len-1 cached decode
        steps with no mask and position = cache length (Q1/Q2); by default no EOS stop: all max_len steps run.  Everything stays on the
        device; returns (tokens [B,max_len] int64, logprob [B] fp32, logits [B,steps_run,V] bf16 | None, state), steps_run == max_len
        without a stop.
        decode_gemm (False | True | "auto"): the steps on the one-pass GEMM step, one decode_gemm + pick per step.
        decode_w8 (False | True): the steps on the e4m3 weight stream (`use_graph` as for the default step).
        stop_on_eos (None | eos_id): the pick marks a row that emits eos_id as finished, freezes its logprob, and raises
        `done` on the device once every row has; the steps are enqueued in chunks of STOP_CHUNK with one look at `done` per chunk
        (`run_generation` on `steps_until_done`: at most 2 * STOP_CHUNK - 1 decode steps are enqueued behind the finishing one, and their picks change nothing).
        A row's tokens up to its EOS, its logprob and its record rows up to that step are bit-equal to the call without a stop (behind its
        EOS a row of a batch that goes on is fed the EOS: other logits); every slot behind a row's EOS holds eos_id; the state (first of the tuple) exposes `steps_run` <= max_len, the rows of the record."""
        B, T, _ = embeds.shape
        w8 = self._use_decode_w8(decode_w8, B, decode_gemm)
        gemm = self._use_decode_gemm(decode_gemm, B)
        eos = check_stop_arg(stop_on_eos, self.cfg.vocab, "generate_greedy")
        keep = None
        if clean_decode_mask and attn_mask is not None:
            keep = torch.ones(B, T + max_len, dtype=torch.uint8, device=self.device)
            keep[:, :T] = (attn_mask != 0).to(self.device, torch.uint8)
        cache, st = self._prefill_for_generation(embeds, attn_mask, max_len, keep_logits, keep, eos_id=eos)
        if gemm:
            def run(n):      # no host synchronisation inside: the step reads the token and the position from the device
                for _ in range(n):
                    self.decode_gemm(cache, st, B)
                    self.pick(cache, st, B, advance_pos=True)
        elif w8:
            run = lambda n: self.greedy_steps_w8(cache, st, B, n, use_graph)
        else:
            run = lambda n: self.greedy_steps(cache, st, B, n, use_graph)
        # (the runner's sync is pcy_ctx_sync: it reads the sticky watchdog word of the fused launches, workgroups not all resident)
        return run_generation(st, max_len, lambda: self.pick(cache, st, B, advance_pos=False), run, self.ctx.sync) + ((st, cache),)

    def decode_window(self, cache: KVCache, st: GenState, embeds, logits):
        """one lookahead pass on the batched decode loop (pcy_llama_decode_window): embeds [W, d] (or [1, W, d]) bf16 -> logits
        [W, V] bf16, K / V of row i appended at slot st.pos + i of the one cache row; st.pos is read on the device and not advanced."""
        _chk_bf16(embeds, logits)
        W = logits.shape[0]
        if embeds.numel() != W * self.cfg.d or tuple(logits.shape) != (W, self.cfg.vocab) or not (embeds.is_contiguous() and logits.is_contiguous()):
            raise ValueError(f"decode_window: embeds {tuple(embeds.shape)} / logits {tuple(logits.shape)} for d {self.cfg.d}, vocab {self.cfg.vocab}")
        L.check(self.ctx.lib.pcy_llama_decode_window(self.ctx.h, C.byref(self.desc), C.byref(cache.c), C.byref(st.c), _p(embeds), W, _p(logits)),
                "pcy_llama_decode_window")

    def look_draft(self, look: "LookState", st: GenState, embeds_out):
        """window[1..W) by prompt lookup + the W embedding rows of the window -> embeds_out [W, d] (pcy_look_draft)"""
        L.check(self.ctx.lib.pcy_look_draft(self.ctx.h, C.byref(self.desc), C.byref(look.c), C.byref(st.c), _p(embeds_out)), "pcy_look_draft")

    def look_verify(self, look: "LookState", st: GenState, logits):
        """pick the W rows of a pass, accept the leading drafts that were right, commit (pcy_look_verify); logits [W, V] bf16"""
        _chk_bf16(logits)
        L.check(self.ctx.lib.pcy_look_verify(self.ctx.h, C.byref(self.desc), C.byref(look.c), C.byref(st.c), _p(logits)), "pcy_look_verify")

    def generate_lookahead(self, embeds, input_ids, max_len, window, ngram=(3, 1), forced=None, keep_logits=False, step="extend", stop_on_eos=None):
        """Greedy generation of ONE prompt with `window - 1` drafted tokens checked per pass over the weights: prefill, token 0
        from its logits as in `generate_greedy`, then passes of draft (prompt lookup over `input_ids` + the text so far, pcy_look_draft) ->
        `extend` of exactly `window` rows at the cache length -> verify + commit (pcy_look_verify) until max_len tokens are committed; by
        default no EOS stop.  embeds [1,T,d] bf16 of an unpadded prompt; input_ids [T] its token ids, negative where a slot holds no text token (soft
        tokens: never matched, never drafted); ngram = (longest, shortest) n-gram looked up; forced: optional [max_len] ints, forced[i] >= 0
        replaces the draft of output token i (tests, measurements).  Returns what `generate_greedy` returns: (tokens [1,max_len] int64,
        logprob [1] fp32, logits [1,max_len,V] bf16 | None, (state, cache, look state)).
        At a fixed window the tokens, the log-prob, the logits record and the K / V of every committed slot do not depend on the drafts; they
        are NOT promised bit-equal to `generate_greedy` (a window-row pass and a one-row decode step are different arithmetic).
        step: what a pass runs on -- "extend" (the default: `extend`, the prefill's launch-per-stage loop) or "window" (`decode_window`, the
        batched decode loop with the window attention; the position is then read on the device).  The two are different
        arithmetic: each is independent of the drafts, they are not promised bit-equal to each other.
        stop_on_eos (None | eos_id): the commit of a pass ends with the first committed token that is eos_id (on the device:
        tokens, logprob and record are those of the call without a stop up to and including the EOS), and the loop, which reads a few bytes
        back per pass anyway, ends with that pass: no pass runs behind the EOS.  Tokens behind the EOS are eos_id, the record is cut to
        [1, steps_run, V], the state exposes `steps_run`."""
        if step not in ("extend", "window"):
            raise ValueError(f"generate_lookahead: step={step!r}: 'extend' or 'window'")
        if embeds.dim() != 3 or embeds.shape[0] != 1:
            raise ValueError(f"generate_lookahead: one prompt at a time, embeds {tuple(embeds.shape)}")
        if embeds.dtype != BF16:
            raise ValueError(f"generate_lookahead needs the bf16 engine, embeds are {embeds.dtype}")
        if bool(self.desc.layers_fp8):
            raise ValueError("generate_lookahead: the cache extension has no fp8 projections (set_fp8(False) first)")
        T, W, max_len = int(embeds.shape[1]), int(window), int(max_len)
        if not 2 <= W <= 32:
            raise ValueError(f"generate_lookahead: window={window} outside [2, 32]")
        ids = torch.as_tensor(input_ids).view(-1)
        if ids.numel() != T:
            raise ValueError(f"generate_lookahead: {ids.numel()} input_ids for {T} prompt slots (one unpadded prompt)")
        if max_len < 1 or T + max_len + W - 1 > self.cfg.max_pos:
            raise ValueError(f"generate_lookahead: T + max_len + window - 1 = {T + max_len + W - 1} exceeds max_pos {self.cfg.max_pos}" if max_len >= 1
                             else f"generate_lookahead: max_len={max_len}")
        g_hi, g_lo = int(ngram[0]), int(ngram[1])
        if not 1 <= g_lo <= g_hi <= 16:
            raise ValueError(f"generate_lookahead: ngram={ngram}: (longest, shortest) with 1 <= shortest <= longest <= 16")
        fz = None
        if forced is not None:
            fz = torch.as_tensor(forced).view(-1).to(torch.int32)
            if fz.numel() != max_len or int(fz.max()) >= self.cfg.vocab:
                raise ValueError(f"generate_lookahead: forced holds {fz.numel()} entries for max_len {max_len}, largest {int(fz.max())} (vocab {self.cfg.vocab})")
        dev, V, d = self.device, self.cfg.vocab, self.cfg.d
        eos = check_stop_arg(stop_on_eos, V, "generate_lookahead")
        # a pass ALWAYS has W rows, also when fewer tokens remain (the projections' tile / K-split choices depend on the row count): the last
        # pass may write up to W - 1 slots beyond the last committed token, hence the spare slots
        cache, st = self._prefill_for_generation(embeds, None, max_len, keep_logits, eos_id=eos, spare_slots=W - 1)
        self.pick(cache, st, 1, advance_pos=False)
        look = LookState(ids, max_len, W, (g_hi, g_lo), dev, fz)
        look.hist[T:T + 1] = st.next_tok
        look.n_hist.fill_(T + 1)
        look.window[0:1] = st.next_tok
        emb = torch.empty(1, W, d, dtype=BF16, device=dev)
        rows = torch.arange(W, dtype=torch.int32, device=dev)
        logits = torch.empty(W, V, dtype=BF16, device=dev)
        on_window = step == "window"      # (`step` counts the committed tokens from here on)
        pos, step = T, 1
        ended = eos is not None and max_len > 1 and bool(int(st.done))      # (token 0 may be the EOS)
        while step < max_len and not ended:
            self.look_draft(look, st, emb)
            # rows of rejected drafts left K / V in slots [pos, pos + W - 1 - accepted) of the previous pass's range: this pass starts at pos,
            # has W rows and so rewrites every one of them before any of its queries reads it (a query at slot p reads [0, p] only)
            if on_window:
                self.decode_window(cache, st, emb, logits)
            else:
                self._extend_call(cache, emb, None, pos, False, rows, logits)
            self.look_verify(look, st, logits)
            # the one host read of a pass: `extend` takes t_past from the host, and either step needs `step` to know when to stop
            # 
            if eos is None:
                _, n, step0, pos0 = look.last.tolist()
            else:
                _, n, step0, pos0, ended = torch.cat([look.last, st.done]).tolist()
            if n < 1:
                raise L.PcyError(f"generate_lookahead: a pass committed nothing at step {step0}")
            pos, step = pos0 + n, step0 + n
        self.ctx.sync()       # the record may live in host memory (as in generate_greedy)
        return hand_out(st) + ((st, cache, look),)

    def generate_beam(self, embeds, attn_mask, max_len, beam_size, group_size, diversity_penalty, eos_id, max_new, decode_gemm=False,
                      shared_attn=False):
        """`_generate_beam_search` (model_unified.py:702-842): diverse beam search of B prompts x beam_size beams, at most max_len tokens, on
        a cache with room for max_new (>= max_len) generated ones.  Returns (tokens [BB,max_len] int64 and scores [BB] on the host, logits
        [BB,steps,V] in pinned host memory), BB = B * beam_size, row r = beam r % beam_size of prompt r // beam_size.
        Nothing synchronises inside a step: the decode step is ONE replayed hipGraph reading the next tokens and the position from device
        memory, the reference's per-group bookkeeping ONE launch (pcy_beam_step), the KV reorder two.  The logits record is kept per SLOT and
        step and re-indexed once at the end along the parent chain (the reference re-indexes the whole history in every group of every step,
        :827-829).  The EOS stop (:833) is decided on the device; the host looks at the flag every 8 steps.
        decode_gemm (False | True | "auto"): the four-call body with the one-pass GEMM step in place of the replayed graph,
        on whichever cache beam_cache_plan chose.
        shared_attn (False | True): the GEMM step's attention scores all beams of a prompt against one pass over its shared prefix
        (`decode_gemm(..., shared_attn=True)`).  ValueError unless this call runs the GEMM step AND beam_cache_plan chose the
        shared cache: there is no fallback.
        shared_attn="split": the split-key attention in whichever step this call runs -- the replayed chain
        (pcy_llama_beam_steps_split), under PCY_DISABLE=beam_graph the four-call body with `decode_split` (same kernels, same bits), with the
        GEMM step `decode_gemm(..., shared_attn="split")`.  ValueError unless beam_cache_plan chose the shared cache: there is no fallback."""
        B, T, _ = embeds.shape
        BB, V, dev = B * beam_size, self.cfg.vocab, self.device
        split = check_shared_attn(shared_attn) == "split"
        off = disabled_switches()
        # Three cache layouts.  Each prompt is prefilled ONCE (the reference replicates it x beam before the prefill, :751-752)
        # and its last-row logits repeated: where beam_cache_plan says so into a B-row cache of exactly T slots that the BB rows share, owning
        # only their max_new suffix slots; otherwise into row b of a BB-row cache, its K / V rows then copied to the rows of its beams (one
        # pcy_kv_reorder, source map r -> r // beam).  PCY_DISABLE=beam_prefill_once, or one beam: the reference's replicated prefill, issued
        # as LlamaPostTokenization.forward issues it (a BB-row batch may take other GEMM tiles than a B-row one: equal to bf16 noise).
        shared = beam_cache_plan(B, beam_size, T, max_new, off)["shared"]
        gemm = self._use_decode_gemm(decode_gemm, BB, shared)
        if split and not shared:
            raise ValueError(f"generate_beam: shared_attn='split' needs the shared-prefix cache (beam_cache_plan -> shared={shared}) for {B} prompts "
                             f"x {beam_size} beams")
        if shared_attn and not split and not (gemm and shared):
            raise ValueError(f"generate_beam: shared_attn needs the GEMM decode step (decode_gemm={decode_gemm!r} -> {gemm}) on the shared-prefix "
                             f"cache (beam_cache_plan -> shared={shared}) for {B} prompts x {beam_size} beams")
        rep = lambda x: x.repeat_interleave(beam_size, dim=0)
        if shared or (beam_size > 1 and "beam_prefill_once" not in off):
            cache = self.new_cache(B, T) if shared else self.new_cache(BB, T + max_new)
            lg_b, _ = self.prefill(embeds.to(dev), attn_mask, cache, "last")
            if shared:
                cache = self.new_beam_cache(cache, beam_size, max_new)
            else:
                self.kv_reorder(cache, torch.arange(BB, dtype=torch.int32) // beam_size, T)
            logits = rep(lg_b).contiguous()
        else:
            cache = self.new_cache(BB, T + max_new)
            logits, _ = self.prefill_all(rep(embeds).to(dev), rep(attn_mask), cache, (torch.arange(BB, dtype=torch.int32) + 1) * T - 1)
        # The beams of a prompt hold the SAME K / V rows in slots [0, T), so the per-step reorder starts at slot T (at 10 beams and a 512-token
        # prompt it was 0.4-0.6 ms of a 4.5 ms step).  PCY_DISABLE=beam_kv_suffix: every slot, as the reference (:830-832; same result).
        kv_t0 = 0 if "beam_kv_suffix" in off or (T * self.cfg.head_dim) % 8 else T
        bs = BeamState(B, beam_size, max_len, eos_id, prompt_len=T, device=dev)
        st = bs.gen_state(V)
        rec = torch.empty(max_len, BB, V, dtype=logits.dtype, device=dev)
        # Step 0 selects on the prefill's logits.  Every later step is decode -> record -> beam step -> KV reorder: ONE replayed launch chain
        # (pcy_llama_beam_steps), enqueued up to the next multiple of 8 steps; PCY_DISABLE=beam_graph: the four calls (same kernels and bits).
        rec[0].copy_(logits)
        self.beam_step(logits, bs, group_size, diversity_penalty)
        self.kv_reorder(cache, bs.src, T, t0=kv_t0)
        def advance(i, n_max):
            if T + i > cache.capacity:
                raise ValueError(f"KV cache capacity {cache.capacity} exhausted; raise max_new_tokens")
            if not (gemm or "beam_graph" in off):
                n = min(n_max, cache.capacity - T - i + 1)
                self.beam_steps(cache, st, bs, group_size, diversity_penalty, rec, n, kv_t0=kv_t0, **({"split": True} if split else {}))
                return n
            if gemm:
                self.decode_gemm(cache, st, BB, **({"shared_attn": shared_attn} if shared_attn else {}))
            elif split:
                self.decode_split(cache, st, BB)
            else:
                self.decode_graph(cache, st, BB)
            rec[i].copy_(st.logits)
            self.beam_step(st.logits, bs, group_size, diversity_penalty)
            self.kv_reorder(cache, bs.src, T + i, t0=kv_t0)
            return 1
        beam_steps_until_done(bs, max_len, advance)
        return beam_hand_out(bs, rec, max_len, self.ctx.sync)      # (the sync raises PcyError for a watchdog of the fused launches)


# ------------------------------------------------------------------------------------------------
@dataclass
class EsmConfig:
    d: int
    n_layers: int
    n_heads: int
    ffn: int
    vocab: int = 33
    ln_eps: float = 1e-5
    rope_theta: float = 10000.0
    rope_math: str = "fp32_once"   # HF Esm; 'model_dtype' = fair-esm's three roundings
    rope_inv_freq_bf16: bool = False
    max_len: int = 1026

    @property
    def head_dim(self):
        return self.d // self.n_heads


PAD_ID, CLS_ID, EOS_ID, MASK_ID = 1, 0, 2, 32


def batched_split_long_seq(toks, padding_idx=1, eos_idx=2, max_protein_len=1024):
    """Host mirror of `batched_split_long_seq(..., "split")` (procyon/training/train_utils.py:1497-1571),
    non-mutating.  toks int64 CPU [B,W] -> (rows [B',max_protein_len+2], keys [B'])."""
    toks = toks.clone()
    W = toks.shape[1]
    cls_idx = int(toks[0, 0])
    add, keys = [], list(range(toks.shape[0]))
    for i in range(toks.shape[0]):
        e = int((toks[i] == eos_idx).nonzero(as_tuple=True)[0][0])
        if e <= max_protein_len + 1:
            continue
        n_add = e // (max_protein_len + 1)
        for j in range(n_add):
            bot = (j + 1) * max_protein_len + 1
            row = torch.full((1, W), padding_idx, dtype=torch.int64)
            tail = toks[i, bot:]
            row[0, 1:tail.shape[0] + 1] = tail
            row[0, 0] = cls_idx
            if j < n_add - 1:
                row[0, max_protein_len + 1] = eos_idx
                row[0, max_protein_len + 2:] = 1
            add.append(row)
            keys.append(i)
        toks[i, max_protein_len + 2:] = padding_idx
        toks[i, max_protein_len + 1] = eos_idx
    new = torch.cat([toks] + add, dim=0)[:, : max_protein_len + 2]
    return new, torch.tensor(keys, dtype=torch.int64)


class EsmEngine:
    """ESM2 encoder + ProteinPooler behind `ESM_PLM.forward` (procyon/model/esm.py:504-558)."""

    def __init__(self, sd, cfg: EsmConfig, device=None, ctx=None):
        self.ctx = ctx or Context.get(device)
        self.cfg = cfg
        dev = self.ctx.device
        self.device = dev
        g = lambda k: sd[k].to(dev, BF16).contiguous()
        self.embed = g("esm.embeddings.word_embeddings.weight")
        self.fw, self.fb = g("esm.encoder.emb_layer_norm_after.weight"), g("esm.encoder.emb_layer_norm_after.bias")
        self.cos, self.sin = rope_tables(cfg.head_dim, cfg.rope_theta, cfg.max_len, dev, cfg.rope_inv_freq_bf16)
        self._keep = []
        self._enc_slots = {}
        arr = (L.EsmLayer * cfg.n_layers)()
        for l in range(cfg.n_layers):
            p = f"esm.encoder.layer.{l}."
            wqkv = torch.cat([g(p + f"attention.self.{n}.weight") for n in ("query", "key", "value")], 0).contiguous()
            bqkv = torch.cat([g(p + f"attention.self.{n}.bias") for n in ("query", "key", "value")], 0).contiguous()
            ts = (wqkv, bqkv, g(p + "attention.output.dense.weight"), g(p + "attention.output.dense.bias"),
                  g(p + "attention.LayerNorm.weight"), g(p + "attention.LayerNorm.bias"),
                  g(p + "intermediate.dense.weight"), g(p + "intermediate.dense.bias"),
                  g(p + "output.dense.weight"), g(p + "output.dense.bias"), g(p + "LayerNorm.weight"), g(p + "LayerNorm.bias"))
            self._keep.append(ts)
            arr[l] = L.EsmLayer(*[t.data_ptr() for t in ts])
        self._arr = arr
        # masked-LM head (fair-esm RobertaLMHead / HF EsmLMHead: dense -> gelu -> layer_norm -> decoder tied to the embedding + bias),
        # only when the checkpoint carries it; consumed by ESM_PLM.forward(aggregate=False) (esm.py:547-558)
        self.lm_head = None
        if "lm_head.dense.weight" in sd:
            dec = sd["lm_head.decoder.weight"] if "lm_head.decoder.weight" in sd else sd["esm.embeddings.word_embeddings.weight"]
            self.lm_head = dict(wd=g("lm_head.dense.weight"), bd=g("lm_head.dense.bias"), lw=g("lm_head.layer_norm.weight"),
                                lb=g("lm_head.layer_norm.bias"), wo=dec.to(dev, BF16).contiguous(), bo=g("lm_head.bias"))
        self.desc = L.EsmDesc(cfg.d, cfg.n_layers, cfg.n_heads, cfg.ffn, cfg.vocab, cfg.ln_eps,
                              1 if cfg.rope_math == "fp32_once" else 0, self.embed.data_ptr(), self.fw.data_ptr(),
                              self.fb.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr(), C.cast(arr, C.POINTER(L.EsmLayer)))

    # = the engine's own bound (pcy_esm_encode; PCY_DISABLE=esm_graph switches the replay off).  Round 5: raised from 4200 (one long protein) to
    # 40 000 tokens (the retrieval batch: 25 x 1026).  A bulk batch is ~230 launches of 25-300 us; on an idle host they are enqueued in 2.4 ms,
    # far ahead of the GPU, but a GPU box whose host cores were busy (other tenants) took ~50 ms per batch for them and the retrieval leg
    # dropped from 634 to 434 proteins/s with the encoder's own time unchanged (profiles/archive/r05_bench.json, history in DESIGN.md): one graph
    # launch per batch takes the host out of the loop.
    GRAPH_MAX_TOKENS = 40000

    def preferred_batch(self, tokens_per_protein, lo=16, hi=40, n_cu=256):
        """Proteins per engine call for retrieval-style bulk encoding ("batch size chosen by the engine", BASELINE configs[2]).
        The four GEMMs of a layer run in rounds of 256 (256 x 256 tiles) or 512 (128 x 128: the o projection) workgroups, so
        throughput follows how well B x S tokens fill the last round of each; beyond ~40 proteins the activations outgrow the
        256 MiB Infinity Cache and throughput declines.  Score = flop-weighted tile-round efficiency - 0.0015 B, fitted on
        ESM2-650M at S = 1026: batch 25 -> 455 proteins/s, 32 -> 419, 26 -> 392, 37 -> 448, 38 -> 434, 64 -> 411."""
        d, F, S = self.cfg.d, self.cfg.ffn, int(tokens_per_protein)
        best, best_score = lo, -1.0
        for B in range(lo, hi + 1):
            M, tot, cost = B * S, 0, 0
            for N, K, t in ((3 * d, d, 256), (d, d, 128 if d < 2560 else 256), (F, d, 256), (d, F, 256)):
                tiles = -(-M // t) * -(-N // t)
                slots = n_cu * (1 if t == 256 else 2)
                cost += -(-tiles // slots) * slots * t * t * K
                tot += M * N * K
            score = tot / cost - 0.0015 * B
            if score > best_score:
                best, best_score = B, score
        return best

    # ---- packing ---------------------------------------------------------------------------------
    @staticmethod
    def pack(rows, mask_pads=True):
        """rows int64 CPU [B',S] (right-padded) -> packed tokens + index arrays (all CPU int32).
        mask_pads=True packs only the non-pad prefix of each row; False keeps pads as tokens (Q12)."""
        Bp, S = rows.shape
        lens = (rows != PAD_ID).sum(1) if mask_pads else torch.full((Bp,), S, dtype=torch.int64)
        real = (rows != PAD_ID).sum(1)
        cu = torch.zeros(Bp + 1, dtype=torch.int64)
        cu[1:] = lens.cumsum(0)
        vt_cu = torch.zeros(Bp + 1, dtype=torch.int64)
        vt_cu[1:] = ((lens + 31) // 32 * 32).cumsum(0)
        idx = torch.arange(S)[None, :] < lens[:, None]
        tokens = rows[idx]
        pos = torch.arange(S)[None, :].expand(Bp, S)[idx]
        return dict(tokens=tokens.to(torch.int32), pos=pos.to(torch.int32), cu=cu.to(torch.int32), vt_cu=vt_cu.to(torch.int32),
                    lens=lens, real=real, ntok=int(cu[-1]), nseq=Bp, max_len=int(lens.max()), vt_total=int(vt_cu[-1]))

    def encode_packed(self, pk, mask_pads=True, borrow=False):
        """borrow=True: the caller consumes the result before the next call of this shape is enqueued (stream order) -- the persistent output
        buffer of a replayed launch chain is returned as it is instead of a copy."""
        dev = self.device
        if pk["max_len"] > self.cfg.max_len:
            raise ValueError(f"sequence of {pk['max_len']} tokens exceeds the rotary table ({self.cfg.max_len})")
        names = ("tokens", "pos", "cu", "vt_cu")
        # Short inputs (one protein: 230 launches of 5-35 us) are replayed from a captured launch chain inside pcy_esm_encode, which
        # needs the SAME device addresses from call to call: persistent index / output buffers per (tokens, sequences), a few shapes kept
        slot = None
        if dev.type == "cuda" and pk["ntok"] <= self.GRAPH_MAX_TOKENS:
            key = (pk["ntok"], pk["nseq"])
            slot = self._enc_slots.pop(key, None)
            if slot is None:
                nbytes = 2 * ((pk["ntok"] * 4 + 255) // 256 * 256) + 2 * (((pk["nseq"] + 1) * 4 + 255) // 256 * 256)
                slot = dict(idx=torch.empty(nbytes, dtype=torch.uint8, device=dev), hidden=torch.empty(pk["ntok"], self.cfg.d, dtype=BF16, device=dev))
            self._enc_slots[key] = slot                      # (most recently used last)
            while len(self._enc_slots) > 8:
                self._enc_slots.pop(next(iter(self._enc_slots)))
        t = dict(zip(names, _h2d_many([pk[k] for k in names], dev, into=None if slot is None else slot["idx"])))
        hidden = torch.empty(pk["ntok"], self.cfg.d, dtype=BF16, device=dev) if slot is None else slot["hidden"]
        L.check(self.ctx.lib.pcy_esm_encode(self.ctx.h, C.byref(self.desc), _p(t["tokens"]), _p(t["pos"]), _p(t["cu"]), _p(t["vt_cu"]),
                                            pk["ntok"], pk["nseq"], pk["max_len"], pk["vt_total"], int(mask_pads), _p(hidden)),
                "pcy_esm_encode")
        return hidden if (slot is None or borrow) else hidden.clone()    # (the persistent buffer is rewritten by the next call of this shape)

    def hidden_states(self, rows, mask_pads=True):
        """rows int64 [B',S] -> padded [B',S,d] representations (pad slots zero-filled; test helper)."""
        pk = self.pack(rows.cpu(), mask_pads)
        h = self.encode_packed(pk, mask_pads)
        Bp, S = rows.shape
        out = torch.zeros(Bp, S, self.cfg.d, dtype=BF16, device=self.device)
        idx = (torch.arange(S)[None, :] < pk["lens"][:, None]).to(self.device)
        out[idx] = h
        return out

    def lm_logits(self, hidden):
        """masked-LM logits [..., vocab] of final-layer states [..., d]: linear + bias -> ESM gelu (op by op, as fair-esm's
        `gelu`) -> LayerNorm -> tied decoder + bias; every Linear / norm rounds to bf16 like the eager reference"""
        if self.lm_head is None:
            raise ValueError("this ESM checkpoint carries no masked-LM head (lm_head.*): logits are not available")
        h = self.lm_head
        x = hidden.reshape(-1, hidden.shape[-1]).contiguous()
        y = self.ctx.gemm(x, h["wd"], bias=h["bd"], epi=L.EPI_GELU_ESM)
        y = self.ctx.layernorm(y, h["lw"], h["lb"], self.cfg.ln_eps)
        out = self.ctx.gemm(y, h["wo"], bias=h["bo"])
        return out.reshape(*hidden.shape[:-1], h["wo"].shape[0])

    def forward_tokens(self, tokens, mask_pads=True, max_protein_len=1024, long_protein_strategy="split", want_logits=True):
        """`ESM_PLM.forward(tokens, aggregate=False)` (esm.py:547-558): per-position final-layer states [B, max_eos + 1, d] (the
        chunks of a split protein laid end to end by `reverse_batched_split`) and, when the checkpoint has the head, the
        masked-LM logits of the same positions.  Pad positions are zero (the reference leaves whatever the padded forward
        computed there; they are masked by every consumer)."""
        from .sequences import reverse_batched_split, split_or_truncate_long_seq
        rows, keys, eos_loc = split_or_truncate_long_seq(tokens.cpu().long(), PAD_ID, EOS_ID, long_protein_strategy, max_protein_len)
        z = self.hidden_states(rows, mask_pads)
        logits = self.lm_logits(z) if (want_logits and self.lm_head is not None) else None
        if keys is not None:
            z = reverse_batched_split(z, keys, eos_loc)
            if logits is not None:
                logits = reverse_batched_split(logits, keys, eos_loc)
        return z, logits

    def forward(self, tokens, pooling="mean", correction=False, mask_pads=True, max_protein_len=1024):
        """`ESM_PLM.forward(tokens, aggregate=True)`: split long proteins, encode, pool per original protein."""
        rows, keys = batched_split_long_seq(tokens.cpu().long(), max_protein_len=max_protein_len)
        pk = self.pack(rows, mask_pads)
        h = self.encode_packed(pk, mask_pads, borrow=True)   # pooled below, on the same stream, before anything can overwrite it
        nprot = int(keys.max()) + 1
        seg = [0]
        rng = []
        for i in range(nprot):
            for r in (keys == i).nonzero(as_tuple=True)[0].tolist():  # chunk rows in batch order (esm.py:168-170)
                rng += [int(pk["cu"][r]), int(pk["real"][r])]          # pads never enter the pool (esm.py:171-173)
            seg.append(len(rng) // 2)
        mode = {"mean": L.POOL_MEAN_CORRECTED if correction else L.POOL_MEAN, "max": L.POOL_MAX}[pooling]
        seg_t, rng_t = _h2d_many([torch.tensor(seg, dtype=torch.int32), torch.tensor(rng, dtype=torch.int32)], self.device)
        return self.ctx.pool(h, seg_t, rng_t, nprot, mode)
