"""fp32 engines: the arithmetic of the reference's callers that never call `.bfloat16()`.

/root/reference/examples/paper_analyses/protpep_qa_scores.py:55-58 (`model.eval(); model.to(device)` -- the loop that defines BASELINE
configs[4]), /root/reference/scripts/qa_filter_captions.py:17-18 and /root/reference/scripts/caption_bulk.py:72-73 run the model as
loaded: fp32 weights, every torch op in fp32.  These engines string the fp32 operator family of libpcy.so (`pcy_f32_*`,
include/pcy.h; procyon_amd/csrc/pcy_f32.hip) together op for op like the reference's modules in that mode:

  EsmEngineF32    ESM2 encoder over packed sequences + ProteinPooler            (/root/reference/procyon/model/esm.py:131-173,504-538)
  MlpEngineF32    `create_mlp` projectors                                        (/root/reference/procyon/model/model_utils.py:13-41)
  LlamaEngineF32  token embedding + soft-token splice, decoder prefill, logits   (/root/reference/procyon/model/pmc_llama.py:546-596,
                  at chosen rows, final hidden states, the L+1-state sum;         /root/reference/procyon/model/model_unified.py:556-581)
                  with a KVCacheF32 also the cached decode step of an fp32
                  generation (`decode`, pcy_f32_attn_decode), the many-token
                  cache extension (`extend`, `extend_behind`, pcy_f32_attn_extend)
                  and HF's causal-LM loss (`score`, pcy_f32_lm_head_xent); opt-in,
                  the device-resident decode step on the streaming fp32 GEMV
                  (`decode_stream`, `greedy_steps`: pcy_f32_llama_decode)
                  and beam search / sampling whose selection runs on the device too
                  (`generate_beam`, `generate_sampling`: pcy_f32_beam_step,
                  pcy_f32_sample_pick and their replayed chains)

The cached decode attends every slot without a mask, as the reference does after the prefill, so it reads the K / V that the prefill
computed from left-pad rows: pcy_f32_attention gives those rows the reference's value (include/pcy.h).  PyTorch holds the device
memory and does index bookkeeping only; every floating-point operation is a HIP kernel behind the C ABI.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .engine import (BeamState, Context, EosStop, EsmConfig, EsmEngine, LlamaConfig, _h2d_many, batched_split_long_seq, beam_hand_out,
                     beam_steps_until_done, check_stop_arg, run_generation, sampling_variates, score_plan, uniform_keep)

F32 = torch.float32


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _chk(*ts):
    for t in ts:
        if t is not None and (t.dtype != F32 or not t.is_cuda or not t.is_contiguous()):
            raise TypeError(f"fp32 engine: expected a contiguous fp32 device tensor, got {t.dtype} {t.device} contiguous={t.is_contiguous()}")


class F32Ops:
    """thin typed wrappers over the pcy_f32_* entry points"""

    def __init__(self, ctx=None, device=None):
        self.ctx = ctx or Context.get(device)
        self.lib, self.h, self.device = self.ctx.lib, self.ctx.h, self.ctx.device

    def linear(self, x, w, bias=None, resid=None, act=0, out=None):
        _chk(x, w, bias, resid)
        M, K = x.shape
        N = w.shape[0]
        out = torch.empty(M, N, dtype=F32, device=x.device) if out is None else out
        L.check(self.lib.pcy_f32_linear(self.h, _p(x), K, _p(w), _p(bias), _p(resid), 0 if resid is None else resid.shape[1], _p(out), N, M, N, K, act),
                "pcy_f32_linear")
        return out

    def layernorm(self, x, w, b, eps):
        _chk(x, w, b)
        y = torch.empty_like(x)
        L.check(self.lib.pcy_f32_layernorm(self.h, _p(x), _p(w), _p(b), _p(y), x.numel() // x.shape[-1], x.shape[-1], eps), "pcy_f32_layernorm")
        return y

    def rmsnorm(self, x, w, eps):
        _chk(x, w)
        y = torch.empty_like(x)
        L.check(self.lib.pcy_f32_rmsnorm(self.h, _p(x), _p(w), _p(y), x.numel() // x.shape[-1], x.shape[-1], eps), "pcy_f32_rmsnorm")
        return y

    def rope(self, buf, col0, nh, dh, pos, cos, sin, prescale=0.0):
        _chk(buf, cos, sin)
        L.check(self.lib.pcy_f32_rope(self.h, _p(buf), buf.shape[1], col0, nh, dh, _p(pos), _p(cos), _p(sin), buf.shape[0], prescale), "pcy_f32_rope")

    def attention(self, q, qcol0, k, kcol0, v, vcol0, cu, keep, nseq, max_len, H, Hkv, dh, causal, scale):
        _chk(q, k, v)
        o = torch.empty(q.shape[0], H * dh, dtype=F32, device=q.device)
        L.check(self.lib.pcy_f32_attention(self.h, _p(q), q.shape[1], qcol0, _p(k), k.shape[1], kcol0, _p(v), v.shape[1], vcol0, _p(o), H * dh,
                                           _p(cu), _p(keep), nseq, max_len, H, Hkv, dh, int(causal), scale), "pcy_f32_attention")
        return o

    def attn_decode(self, q, kcache, vcache, nkeys, H, Hkv, dh, scale):
        """q [B, H*dh] (a view with row stride q.stride(0) is fine) against slots [0, nkeys) of token-major caches [B, Tmax, Hkv*dh]"""
        _chk(kcache, vcache)
        if q.dtype != F32 or not q.is_cuda or q.dim() != 2 or q.stride(1) != 1 or q.stride(0) % 4:
            raise TypeError(f"fp32 engine: q must be an fp32 device matrix with unit inner stride and a row stride that is a multiple of 4 "
                            f"floats, got {q.dtype} {q.device} strides {tuple(q.stride())}")
        B = q.shape[0]
        o = torch.empty(B, H * dh, dtype=F32, device=q.device)
        L.check(self.lib.pcy_f32_attn_decode(self.h, _p(q), q.stride(0), _p(kcache), _p(vcache), kcache.shape[2], kcache.shape[1], _p(o), H * dh, B,
                                             H, Hkv, dh, nkeys, scale), "pcy_f32_attn_decode")
        return o

    def gemv(self, x, w, w2=None, resid=None, epi=L.EPI_STORE, out=None):
        """the streaming fp32 GEMV (pcy_f32_gemv): y[b] = epi(x[b] . w^T); x [B, K], out / resid [B, N] may be column windows of wider
        buffers (row strides that are multiples of 4 floats for x); w [N, K]; epi EPI_STORE, EPI_RESID (y = v + resid, resid may be `out`) or
        EPI_SWIGLU (y = silu(x . w^T) * (x . w2^T), two separate matrices)"""
        _chk(w, w2)
        self._chk_rows(x, "x")
        B, K = x.shape
        N = w.shape[0]
        if w.dim() != 2 or w.shape[1] != K or (w2 is not None and w2.shape != w.shape):
            raise TypeError(f"fp32 engine: w {tuple(w.shape)} / w2 {None if w2 is None else tuple(w2.shape)} do not match x {tuple(x.shape)}")
        out = torch.empty(B, N, dtype=F32, device=x.device) if out is None else out
        for t, what in ((out, "out"), (resid, "resid")):
            if t is not None and (t.dtype != F32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or tuple(t.shape) != (B, N)):
                raise TypeError(f"fp32 engine: {what} must be an fp32 device matrix [{B}, {N}] with unit inner stride")
        ld = lambda t: t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
        L.check(self.lib.pcy_f32_gemv(self.h, _p(w), _p(w2), _p(x), ld(x), _p(resid), 0 if resid is None else ld(resid), _p(out), ld(out), N, K, B,
                                      int(epi)), "pcy_f32_gemv")
        return out

    def attn_decode_pos(self, qkv, kcache, vcache, pos, cos, sin, H, Hkv, dh, scale, out=None):
        """pcy_f32_attn_decode_pos: qkv [B, >= (H + 2 Hkv) dh] un-roped (not written), token-major caches [B, Tmax, Hkv*dh], pos an int32
        device scalar = cache length = rotary position: ropes q / the new k, appends K / V at slot *pos, attends slots [0, *pos] -> o [B, H*dh]"""
        _chk(kcache, vcache, cos, sin)
        self._chk_rows(qkv, "qkv", (H + 2 * Hkv) * dh)
        if pos.dtype != torch.int32 or not pos.is_cuda or pos.numel() != 1:
            raise TypeError("fp32 engine: pos must be an int32 device scalar")
        if kcache.dim() != 3 or kcache.shape != vcache.shape or kcache.shape[0] < qkv.shape[0]:
            raise TypeError(f"fp32 engine: caches must be [>= {qkv.shape[0]}, Tmax, ldkv], got {tuple(kcache.shape)} / {tuple(vcache.shape)}")
        B = qkv.shape[0]
        o = torch.empty(B, H * dh, dtype=F32, device=qkv.device) if out is None else out
        ld = qkv.stride(0) if B > 1 else max(qkv.stride(0), qkv.shape[1])
        L.check(self.lib.pcy_f32_attn_decode_pos(self.h, _p(qkv), ld, _p(kcache), _p(vcache), kcache.shape[2], kcache.shape[1], _p(o), o.stride(0) if B > 1 else H * dh,
                                                 _p(pos), _p(cos), _p(sin), B, H, Hkv, dh, scale), "pcy_f32_attn_decode_pos")
        return o

    @staticmethod
    def _chk_rows(t, what, min_cols=0):
        """an fp32 device matrix whose rows the 16-byte loads can read: unit inner stride, row stride and base address multiples of 4 floats"""
        if (not isinstance(t, torch.Tensor) or t.dtype != F32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) % 4
                or t.data_ptr() % 16 or t.shape[1] < min_cols):
            raise TypeError(f"fp32 engine: {what} must be an fp32 device matrix with unit inner stride, a row stride that is a multiple of 4 floats and a "
                            f"16-byte aligned base, got {getattr(t, 'dtype', type(t))} {getattr(t, 'device', None)} shape "
                            f"{tuple(getattr(t, 'shape', ()))} strides {tuple(t.stride()) if isinstance(t, torch.Tensor) else None}")

    def attn_extend(self, qkv, S, kcache, vcache, t_past, H, Hkv, dh, scale, keep=None, cache_rows=None):
        """S new query rows per row: qkv [B*S, >= (H + 2 Hkv) dh] roped (q | new K | new V, row b*S + s; a view with a row stride is fine)
        against slots [0, t_past) of token-major caches [rows, Tmax, Hkv*dh] and the new keys 0..s of the row itself.  keep uint8
        [B, >= t_past + S] (0 = masked key) or None; cache_rows int32 [B] (row b reads cache row cache_rows[b]) or None = b.  -> o [B*S, H*dh]"""
        _chk(kcache, vcache)
        self._chk_rows(qkv, "qkv", (H + 2 * Hkv) * dh)
        S = int(S)
        if S < 1 or qkv.shape[0] % S:
            raise ValueError(f"qkv holds {qkv.shape[0]} rows: not a multiple of S = {S}")
        B = qkv.shape[0] // S
        ld = qkv.stride(0) if qkv.shape[0] > 1 else qkv.shape[1]
        if kcache.dim() != 3 or kcache.shape != vcache.shape or kcache.shape[2] != Hkv * dh:
            raise TypeError(f"fp32 engine: caches must be [rows, Tmax, {Hkv * dh}], got {tuple(kcache.shape)} / {tuple(vcache.shape)}")
        nrows, Tmax = kcache.shape[0], kcache.shape[1]
        if cache_rows is not None:
            if cache_rows.dtype != torch.int32 or not cache_rows.is_cuda or not cache_rows.is_contiguous() or cache_rows.numel() != B:
                raise TypeError("fp32 engine: cache_rows must be a contiguous int32 device tensor [B]")
            if B and (int(cache_rows.min()) < 0 or int(cache_rows.max()) >= nrows):
                raise ValueError(f"cache_rows outside the {nrows} rows of the cache")
        elif B > nrows:
            raise ValueError(f"{B} rows on a cache of {nrows}")
        ldkeep = 0
        if keep is not None:
            if keep.dtype != torch.uint8 or not keep.is_cuda or keep.dim() != 2 or keep.stride(1) != 1 or keep.shape[0] != B or keep.shape[1] < t_past + S:
                raise TypeError(f"fp32 engine: keep must be a uint8 device matrix [{B}, >= {t_past + S}] with unit inner stride")
            ldkeep = keep.stride(0) if B > 1 else keep.shape[1]
        o = torch.empty(B * S, H * dh, dtype=F32, device=qkv.device)
        L.check(self.lib.pcy_f32_attn_extend(self.h, _p(qkv), ld, _p(kcache), _p(vcache), kcache.shape[2], Tmax, _p(cache_rows), _p(keep), ldkeep,
                                             _p(o), H * dh, B, S, int(t_past), H, Hkv, dh, scale), "pcy_f32_attn_extend")
        return o

    def lm_head_xent(self, x, W, targets, want_parts=False):
        """nll [M] fp32 = logsumexp(x . W^T) - (x . W^T)[targets] without the [M, V] logits (pcy_f32_lm_head_xent); x [M, d] fp32 (a view with
        a row stride is fine), W [V, d], targets int32 [M] on the device.  want_parts: (nll, lse, row_max, label_logit)."""
        _chk(W)
        self._chk_rows(x, "x")
        if W.dim() != 2 or W.shape[1] != x.shape[1]:
            raise TypeError(f"fp32 engine: W {tuple(W.shape)} does not match x {tuple(x.shape)}")
        M, d = x.shape
        V = W.shape[0]
        if targets.dtype != torch.int32 or not targets.is_cuda or not targets.is_contiguous() or targets.numel() != M:
            raise TypeError("fp32 engine: targets must be a contiguous int32 device tensor [M]")
        outs = [torch.empty(M, dtype=F32, device=x.device) for _ in range(4 if want_parts else 1)]
        ldx = x.stride(0) if M > 1 else d
        L.check(self.lib.pcy_f32_lm_head_xent(self.h, _p(x), ldx, _p(W), M, V, d, _p(targets), *[_p(t) for t in outs], *([None] * (4 - len(outs)))),
                "pcy_f32_lm_head_xent")
        return tuple(outs) if want_parts else outs[0]

    def lm_head_xent_ws_bytes(self, M, V):
        return int(self.lib.pcy_f32_lm_head_xent_ws_bytes(int(M), int(V)))

    def embed(self, table, ids, soft=None, soft_map=None):
        _chk(table, soft)
        out = torch.empty(ids.numel(), table.shape[1], dtype=F32, device=table.device)
        L.check(self.lib.pcy_f32_embed(self.h, _p(table), _p(ids), _p(soft), _p(soft_map), _p(out), ids.numel(), table.shape[1]), "pcy_f32_embed")
        return out

    def silu_mul(self, g, u):
        _chk(g, u)
        o = torch.empty_like(g)
        L.check(self.lib.pcy_f32_silu_mul(self.h, _p(g), _p(u), _p(o), g.numel()), "pcy_f32_silu_mul")
        return o

    def acc_rows(self, dst, src, rows):
        _chk(dst, src)
        L.check(self.lib.pcy_f32_acc_rows(self.h, _p(src), src.shape[-1], _p(rows), _p(dst), rows.numel(), src.shape[-1]), "pcy_f32_acc_rows")


def _rope_tables_f32(dh, theta, n_pos, device):
    inv_freq = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.float32) / dh))
    pos = torch.arange(n_pos, dtype=torch.float32)
    freqs = (inv_freq[:, None] @ pos[None, :]).transpose(0, 1)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(device).contiguous(), emb.sin().to(device).contiguous()


class MlpEngineF32:
    """`create_mlp` in eval mode: Linear(+bias) -> GELU ... -> Linear(+bias); one bias-free Linear when n_layers == 1"""

    def __init__(self, layers, ctx=None, device=None):
        self.ops = F32Ops(ctx, device)
        dev = self.ops.device
        self.layers = [(w.to(dev, F32).contiguous(), None if b is None else b.to(dev, F32).contiguous()) for w, b in layers]
        self.in_features, self.out_features = self.layers[0][0].shape[1], self.layers[-1][0].shape[0]

    def __call__(self, x):
        shape = x.shape
        x = x.reshape(-1, shape[-1]).to(self.ops.device, F32).contiguous()
        n = len(self.layers)
        for i, (w, b) in enumerate(self.layers):
            if x.shape[0]:
                x = self.ops.linear(x, w, b, act=1 if i < n - 1 else 0)
            else:
                x = torch.empty(0, w.shape[0], dtype=F32, device=x.device)
        return x.reshape(*shape[:-1], self.out_features)


class EsmEngineF32:
    """ESM2 (HF layout state dict, fp32) over packed varlen sequences + ProteinPooler; same call surface as `EsmEngine.forward`."""

    def __init__(self, sd, cfg: EsmConfig, device=None, ctx=None):
        self.ops = F32Ops(ctx, device)
        self.cfg, self.device = cfg, self.ops.device
        g = lambda k: sd[k].to(self.device, F32).contiguous()
        self.embed = g("esm.embeddings.word_embeddings.weight")
        self.fw, self.fb = g("esm.encoder.emb_layer_norm_after.weight"), g("esm.encoder.emb_layer_norm_after.bias")
        self.cos, self.sin = _rope_tables_f32(cfg.head_dim, cfg.rope_theta, cfg.max_len, self.device)
        self.layers = []
        for l in range(cfg.n_layers):
            p = f"esm.encoder.layer.{l}."
            self.layers.append(dict(
                wqkv=torch.cat([g(p + f"attention.self.{n}.weight") for n in ("query", "key", "value")], 0).contiguous(),
                bqkv=torch.cat([g(p + f"attention.self.{n}.bias") for n in ("query", "key", "value")], 0).contiguous(),
                wo=g(p + "attention.output.dense.weight"), bo=g(p + "attention.output.dense.bias"),
                ln1w=g(p + "attention.LayerNorm.weight"), ln1b=g(p + "attention.LayerNorm.bias"),
                w1=g(p + "intermediate.dense.weight"), b1=g(p + "intermediate.dense.bias"),
                w2=g(p + "output.dense.weight"), b2=g(p + "output.dense.bias"), ln2w=g(p + "LayerNorm.weight"), ln2b=g(p + "LayerNorm.bias")))

    def encode_packed(self, pk, mask_pads=True):
        ops, cfg = self.ops, self.cfg
        if pk["max_len"] > cfg.max_len:
            raise ValueError(f"sequence of {pk['max_len']} tokens exceeds the rotary table ({cfg.max_len})")
        tokens, pos, cu = _h2d_many([pk["tokens"], pk["pos"], pk["cu"]], self.device)
        d, H, dh = cfg.d, cfg.n_heads, cfg.head_dim
        x = torch.empty(pk["ntok"], d, dtype=F32, device=self.device)
        L.check(ops.lib.pcy_f32_esm_embed(ops.h, _p(self.embed), _p(tokens), _p(cu), pk["nseq"], pk["max_len"], _p(x), d, int(mask_pads)), "pcy_f32_esm_embed")
        for lw in self.layers:
            xn = ops.layernorm(x, lw["ln1w"], lw["ln1b"], cfg.ln_eps)
            qkv = ops.linear(xn, lw["wqkv"], lw["bqkv"])
            ops.rope(qkv, 0, H, dh, pos, self.cos, self.sin, prescale=dh ** -0.5)       # q * dh^-1/2, then rotated (esm2 attention)
            ops.rope(qkv, d, H, dh, pos, self.cos, self.sin)
            ao = ops.attention(qkv, 0, qkv, d, qkv, 2 * d, cu, None, pk["nseq"], pk["max_len"], H, H, dh, False, 1.0)
            x = ops.linear(ao, lw["wo"], lw["bo"], resid=x)
            xn = ops.layernorm(x, lw["ln2w"], lw["ln2b"], cfg.ln_eps)
            act = ops.linear(xn, lw["w1"], lw["b1"], act=1)
            x = ops.linear(act, lw["w2"], lw["b2"], resid=x)
        return ops.layernorm(x, self.fw, self.fb, cfg.ln_eps)

    def hidden_states(self, rows, mask_pads=True):
        """rows int64 [B',S] -> padded [B',S,d] representations (pad slots zero-filled; test helper)"""
        pk = EsmEngine.pack(rows.cpu(), mask_pads)
        h = self.encode_packed(pk, mask_pads)
        Bp, S = rows.shape
        out = torch.zeros(Bp, S, self.cfg.d, dtype=F32, device=self.device)
        out[(torch.arange(S)[None, :] < pk["lens"][:, None]).to(self.device)] = h
        return out

    def forward(self, tokens, pooling="mean", correction=False, mask_pads=True, max_protein_len=1024):
        """`ESM_PLM.forward(tokens, aggregate=True)` in fp32: split long proteins, encode, pool per original protein"""
        rows, keys = batched_split_long_seq(tokens.cpu().long(), max_protein_len=max_protein_len)
        pk = EsmEngine.pack(rows, mask_pads)
        h = self.encode_packed(pk, mask_pads)
        nprot = int(keys.max()) + 1
        seg, rng = [0], []
        for i in range(nprot):
            for r in (keys == i).nonzero(as_tuple=True)[0].tolist():
                rng += [int(pk["cu"][r]), int(pk["real"][r])]
            seg.append(len(rng) // 2)
        mode = {"mean": L.POOL_MEAN_CORRECTED if correction else L.POOL_MEAN, "max": L.POOL_MAX}[pooling]
        seg_t, rng_t = _h2d_many([torch.tensor(seg, dtype=torch.int32), torch.tensor(rng, dtype=torch.int32)], self.device)
        out = torch.empty(nprot, self.cfg.d, dtype=F32, device=self.device)
        L.check(self.ops.lib.pcy_f32_pool(self.ops.h, _p(h), self.cfg.d, _p(seg_t), _p(rng_t), nprot, mode, _p(out)), "pcy_f32_pool")
        return out


def _no_shared_prefix(cache):
    """the fp32 family reads plain caches only (a shared-prefix cache, engine.KVCache with a prefix, belongs to the bf16 batched decode loop)"""
    if getattr(cache, "prefix", None) is not None:
        raise ValueError("the fp32 decoder does not take a cache with a shared prefix")


class KVCacheF32:
    """token-major fp32 K (roped) / V caches [L, B, Tmax, Hkv*dh]"""

    def __init__(self, cfg: LlamaConfig, B, Tmax, device):
        kw = cfg.n_kv_heads * cfg.head_dim
        self.k = torch.zeros(cfg.n_layers, B, Tmax, kw, dtype=F32, device=device)
        self.v = torch.zeros(cfg.n_layers, B, Tmax, kw, dtype=F32, device=device)
        self.B, self.Tmax = B, Tmax

    def reorder_(self, src_rows, t=None):
        """row b takes the cache of row src_rows[b] (beam search, model_unified.py:830-832) -- in place, only the rows that move and only the
        `t` slots written so far (all of them when t is None): a beam-10 x batch-8 search at 900 slots used to rebuild 2 x 9 GB per step"""
        idx = src_rows.to(self.k.device).long()
        moved = (idx != torch.arange(idx.numel(), device=idx.device)).nonzero(as_tuple=True)[0]
        if moved.numel() == 0:
            return
        t = self.Tmax if t is None else min(int(t), self.Tmax)
        for c in (self.k, self.v):
            c[:, moved, :t] = c[:, idx[moved], :t]       # (advanced indexing on the right gathers into a temporary first: sources are read before any write)


class GenStateF32(EosStop):
    """device state of the fp32 stream step (a pcy_gen_state whose logits hold fp32): pos / step int32 scalars, next_tok [B], tokens_out
    [B, max_steps], logprob [B], logits [B, V], optionally the record logits_all [max_steps, B, V].  pos / next_tok: arrays to share
    instead of new ones (a beam search: the step reads what the beam step writes, as engine.BeamState.gen_state does for bf16).  eos_id: the
    EOS stop of the greedy and sampling picks (engine.EosStop; None: no stop, nothing allocated)"""

    def __init__(self, B, vocab, max_steps, device, keep_logits=False, pos=None, next_tok=None, eos_id=None):
        i32 = dict(dtype=torch.int32, device=device)
        self.B, self.vocab, self.max_steps = B, vocab, max_steps
        self.pos, self.step = torch.zeros(1, **i32) if pos is None else pos, torch.zeros(1, **i32)
        self.next_tok = torch.zeros(B, **i32) if next_tok is None else next_tok
        self.tokens_out = torch.zeros(B, max_steps, **i32)
        self.logprob = torch.zeros(B, dtype=F32, device=device)
        self.logits = torch.zeros(B, vocab, dtype=F32, device=device)
        self.logits_all = torch.zeros(max_steps, B, vocab, dtype=F32, device=device) if keep_logits else None
        self._init_stop(B, eos_id, device, max_steps)
        self.c = L.GenState(_p(self.pos), _p(self.step), _p(self.next_tok), _p(self.tokens_out), _p(self.logprob), _p(self.logits), _p(self.logits_all),
                            None, max_steps, 0, *self._stop_args())

    def set(self, pos=None, step=None, next_tok=None):
        """device-side writes only (a fill / a copy on the stream: nothing is read back)"""
        if pos is not None:
            self.pos.fill_(int(pos))
        if step is not None:
            self.step.fill_(int(step))
        if next_tok is not None:
            self.next_tok.copy_(next_tok.reshape(-1).to(torch.int32), non_blocking=True)


class LlamaEngineF32:
    """Llama decoder in fp32 (HF layout state dict): embedding + splice, L layers, final norm, logits at chosen rows; with a cache also
    the KV-cached decode step (`decode`: one launch per operator, 82 ms per step at full size) and, opt-in, the device-resident step that streams
    the fp32 weights once per step and is replayed as a graph (`decode_stream` / `greedy_steps`, 8.4-13.7 ms; other bits than `decode`)."""

    def __init__(self, sd, cfg: LlamaConfig, device=None, ctx=None):
        self.ops = F32Ops(ctx, device)
        self.cfg, self.device = cfg, self.ops.device
        g = lambda k: sd[k].to(self.device, F32).contiguous()
        self.embed = g("model.embed_tokens.weight")
        self.final_norm = g("model.norm.weight")
        self.lm_head = g("lm_head.weight")
        self.cos, self.sin = _rope_tables_f32(cfg.head_dim, cfg.rope_theta, cfg.max_pos, self.device)
        self.layers = []
        for l in range(cfg.n_layers):
            p = f"model.layers.{l}."
            self.layers.append(dict(
                wqkv=torch.cat([g(p + f"self_attn.{n}_proj.weight") for n in "qkv"], 0).contiguous(), wo=g(p + "self_attn.o_proj.weight"),
                wg=g(p + "mlp.gate_proj.weight"), wu=g(p + "mlp.up_proj.weight"), wd=g(p + "mlp.down_proj.weight"),
                ln1=g(p + "input_layernorm.weight"), ln2=g(p + "post_attention_layernorm.weight")))

    def embed_tokens(self, ids, soft=None, soft_map=None):
        """[B,T] ids (+ soft tokens [n,d] fp32 and a flat row -> soft index map, -1 = a table row) -> [B,T,d] fp32"""
        B, T = ids.shape
        ids_d, = _h2d_many([ids.reshape(-1).to(torch.int32).cpu()], self.device)
        sm = None
        if soft_map is not None:
            sm, = _h2d_many([soft_map.reshape(-1).to(torch.int32).cpu()], self.device)
            soft = soft.to(self.device, F32).contiguous()
        return self.ops.embed(self.embed, ids_d, soft if soft_map is not None else None, sm).view(B, T, self.cfg.d)

    def new_cache(self, B, Tmax):
        return KVCacheF32(self.cfg, B, Tmax, self.device)

    def decode(self, cache: KVCacheF32, ids, t):
        """one new token per row (ids [B]) at cache length / rotary position t for EVERY row, no mask (reference quirks Q1 / Q2,
        model_unified.py:769, :887) -> logits [B, V] fp32; appends K / V at slot t"""
        ops, cfg = self.ops, self.cfg
        H, Hkv, dh = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        B = ids.numel()
        _no_shared_prefix(cache)
        if t + 1 > cache.Tmax:
            raise ValueError(f"KV cache capacity {cache.Tmax} exhausted; raise max_new_tokens")
        ids_d, = _h2d_many([ids.reshape(-1).to(torch.int32).cpu()], self.device)
        x = ops.embed(self.embed, ids_d)
        pos = torch.full((B,), t, dtype=torch.int32, device=self.device)
        qw, kw = H * dh, Hkv * dh
        for l, lw in enumerate(self.layers):
            xn = ops.rmsnorm(x, lw["ln1"], cfg.rms_eps)
            qkv = ops.linear(xn, lw["wqkv"])
            ops.rope(qkv, 0, H, dh, pos, self.cos, self.sin)
            ops.rope(qkv, qw, Hkv, dh, pos, self.cos, self.sin)
            cache.k[l, :, t] = qkv[:, qw:qw + kw]
            cache.v[l, :, t] = qkv[:, qw + kw:]
            ao = ops.attn_decode(qkv, cache.k[l], cache.v[l], t + 1, H, Hkv, dh, dh ** -0.5)
            x = ops.linear(ao, lw["wo"], resid=x)
            xn = ops.rmsnorm(x, lw["ln2"], cfg.rms_eps)
            act = ops.silu_mul(ops.linear(xn, lw["wg"]), ops.linear(xn, lw["wu"]))
            x = ops.linear(act, lw["wd"], resid=x)
        return ops.linear(ops.rmsnorm(x, self.final_norm, cfg.rms_eps), self.lm_head)

    # ---- the device-resident step on the streaming fp32 GEMV (pcy_f32_llama_decode): opt-in beside `decode`, other bits
    def _stream_desc(self):
        if getattr(self, "_sdesc", None) is None:
            cfg = self.cfg
            arr = (L.LlamaLayerF32 * cfg.n_layers)(*[L.LlamaLayerF32(*[lw[n].data_ptr() for n in ("wqkv", "wo", "wg", "wu", "wd", "ln1", "ln2")])
                                                     for lw in self.layers])
            self._sdesc_layers = arr       # (the descriptor points into it: kept alive with the engine)
            self._sdesc = L.LlamaDescF32(cfg.vocab, cfg.d, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.ffn, cfg.max_pos, cfg.rms_eps,
                                         self.embed.data_ptr(), self.final_norm.data_ptr(), self.lm_head.data_ptr(), self.cos.data_ptr(),
                                         self.sin.data_ptr(), arr)
        return self._sdesc

    def new_gen_state(self, B, max_steps, keep_logits=False, eos_id=None):
        return GenStateF32(B, self.cfg.vocab, max_steps, self.device, keep_logits, eos_id=eos_id)

    @staticmethod
    def _stream_cache(cache):
        _no_shared_prefix(cache)
        c = L.KvCacheF32(cache.k.data_ptr(), cache.v.data_ptr(), cache.B, cache.Tmax)
        return c

    def decode_stream(self, cache: KVCacheF32, st: GenStateF32, B, graph=True):
        """one step for rows [0, B): st.next_tok at position *st.pos (both read on the device) -> st.logits [B, V] fp32, K / V appended at slot
        *st.pos; no pick, no advance, no host read.  graph: replay the captured chain (same bits as the eager launches)."""
        fn = self.ops.lib.pcy_f32_llama_decode_graph if graph else self.ops.lib.pcy_f32_llama_decode
        L.check(fn(self.ops.h, C.byref(self._stream_desc()), C.byref(self._stream_cache(cache)), C.byref(st.c), int(B)),
                "pcy_f32_llama_decode_graph" if graph else "pcy_f32_llama_decode")
        return st.logits[:B]

    def greedy_pick(self, cache, st, B, advance_pos=True):
        L.check(self.ops.lib.pcy_f32_greedy_pick(self.ops.h, C.byref(self._stream_desc()), C.byref(self._stream_cache(cache)), C.byref(st.c), int(B),
                                                 int(bool(advance_pos))), "pcy_f32_greedy_pick")

    def greedy_steps(self, cache: KVCacheF32, st: GenStateF32, B, n_steps, graph=True):
        """n_steps x (step + greedy pick + advance) on the device without a host synchronisation (pcy_f32_llama_greedy)"""
        L.check(self.ops.lib.pcy_f32_llama_greedy(self.ops.h, C.byref(self._stream_desc()), C.byref(self._stream_cache(cache)), C.byref(st.c), int(B),
                                                  int(n_steps), int(bool(graph))), "pcy_f32_llama_greedy")

    # ---- selection on the device: the beam step, the K / V rows that follow the parents, the sampling pick, their chains
    def beam_step(self, logits, bs: BeamState, group_size, diversity_penalty):
        """one step of the diverse-beam bookkeeping on fp32 logits [BB, V] (pcy_f32_beam_step; engine.BeamState holds the state)"""
        _chk(logits)
        L.check(self.ops.lib.pcy_f32_beam_step(self.ops.h, _p(logits), logits.shape[1], bs.B, bs.beam, int(group_size), float(diversity_penalty),
                                               C.byref(bs.c)), "pcy_f32_beam_step")

    def kv_reorder(self, cache: KVCacheF32, src_rows, t, t0=0):
        """cache[:, b] = cache[:, src_rows[b]] over slots [t0, t), in place, any map (pcy_f32_kv_reorder_range)"""
        src = src_rows.to(self.device, torch.int32).contiguous()
        L.check(self.ops.lib.pcy_f32_kv_reorder_range(self.ops.h, C.byref(self._stream_desc()), C.byref(self._stream_cache(cache)), _p(src),
                                                      src.numel(), int(t0), int(t)), "pcy_f32_kv_reorder_range")

    def kv_copy_rows(self, dst: KVCacheF32, src: KVCacheF32, src_rows, t):
        """dst[:, r, :t] = src[:, src_rows[r], :t] for the rows of the map (pcy_f32_kv_copy_rows): a B-row prefill into B * beam rows"""
        rows = src_rows.to(self.device, torch.int32).contiguous()
        L.check(self.ops.lib.pcy_f32_kv_copy_rows(self.ops.h, C.byref(self._stream_desc()), C.byref(self._stream_cache(dst)),
                                                  C.byref(self._stream_cache(src)), _p(rows), rows.numel(), int(t)), "pcy_f32_kv_copy_rows")

    def beam_steps(self, cache: KVCacheF32, st: GenStateF32, bs: BeamState, group_size, diversity_penalty, logits_rec, n_steps, kv_t0=0):
        """n_steps x (step -> record -> beam step -> reorder of [kv_t0, *pos)), each ONE replayed launch chain (pcy_f32_llama_beam_steps);
        st.pos / st.next_tok are the beam state's arrays"""
        _chk(logits_rec)
        L.check(self.ops.lib.pcy_f32_llama_beam_steps(self.ops.h, C.byref(self._stream_desc()), C.byref(self._stream_cache(cache)), C.byref(st.c),
                                                      bs.B, bs.beam, int(group_size), float(diversity_penalty), C.byref(bs.c), _p(logits_rec),
                                                      int(n_steps), int(kv_t0)), "pcy_f32_llama_beam_steps")

    def sample_pick(self, cache, st: GenStateF32, B, advance_pos, uniforms, temperature=1.0, nucleus_prob=None, probs_out=None):
        """sampling / nucleus selection on st.logits with the variates uniforms[step * B + b] (pcy_f32_sample_pick)"""
        _chk(uniforms, probs_out)
        L.check(self.ops.lib.pcy_f32_sample_pick(self.ops.h, C.byref(self._stream_desc()), C.byref(self._stream_cache(cache)), C.byref(st.c), int(B),
                                                 int(bool(advance_pos)), float(temperature), -1.0 if nucleus_prob is None else float(nucleus_prob),
                                                 _p(uniforms), _p(probs_out)), "pcy_f32_sample_pick")

    def sample_steps(self, cache, st: GenStateF32, B, n_steps, uniforms, temperature=1.0, nucleus_prob=None, graph=True):
        """n_steps x (step + sampling pick + advance) on the device without a host synchronisation (pcy_f32_llama_sample)"""
        _chk(uniforms)
        L.check(self.ops.lib.pcy_f32_llama_sample(self.ops.h, C.byref(self._stream_desc()), C.byref(self._stream_cache(cache)), C.byref(st.c), int(B),
                                                  int(n_steps), float(temperature), -1.0 if nucleus_prob is None else float(nucleus_prob),
                                                  _p(uniforms), int(bool(graph))), "pcy_f32_llama_sample")

    def select_count(self, which):
        """steps enqueued by the selection entries -- 0: beam, 1: sampling (pcy_debug_f32_select_count)"""
        return int(self.ops.lib.pcy_debug_f32_select_count(int(which)))

    def _generation_capacity(self, T, max_len, max_new):
        """slots of a cache for a T-token prompt and max_new generated tokens, inside the rotary table; ValueError when max_len tokens need more"""
        Tmax = min(T + max(int(max_new), 1), self.cfg.max_pos)
        if T + max_len - 1 > Tmax:
            raise ValueError(f"KV cache capacity {Tmax} exhausted by a {T}-token prompt and {max_len} generated tokens; raise max_new_tokens")
        return Tmax

    def generate_beam(self, embeds, attn_mask, max_len, beam_size, group_size, diversity_penalty, eos_id, max_new):
        """`_generate_beam_search` (model_unified.py:702-842) of an fp32 model with nothing but the 8-step look at `done` on the host: diverse
        beam search of B prompts x beam_size beams, at most max_len tokens, on a cache with room for max_new generated ones.  Returns what
        `LlamaEngine.generate_beam` returns -- (tokens [BB, max_len] int64 and scores [BB] on the host, logits [BB, steps, V] fp32 in pinned
        host memory), BB = B * beam_size, row r = beam r % beam_size of prompt r // beam_size.
        ONE fp32 prefill of the B prompts into a B-row cache, its rows copied to the rows of their beams (kv_copy_rows, map r // beam; the
        reference replicates the prompts before the prefill, :751-752); step 0 on the repeated prefill logits; then `beam_steps` up to the
        next multiple of 8 steps.  The beams of a prompt hold the same K / V rows below slot T, so the per-step reorder starts there.  The
        logits record is kept per slot on the device and re-indexed once along the parent chain at the end.  ValueError before any decode
        step when max_len tokens do not fit the cache."""
        B, T, _ = embeds.shape
        BB, V, dev = B * beam_size, self.cfg.vocab, self.device
        if beam_size > 32 or beam_size < 1 or group_size < 1 or beam_size % group_size:
            raise ValueError(f"generate_beam: beam_size={beam_size} (1..32) must be a multiple of group_size={group_size}")
        Tmax = self._generation_capacity(T, max_len, max_new)
        small = self.new_cache(B, T)
        lg_b, _ = self.prefill(embeds, attn_mask, "last", cache=small)
        cache = self.new_cache(BB, Tmax)
        self.kv_copy_rows(cache, small, torch.arange(BB, dtype=torch.int32) // beam_size, T)
        logits = lg_b.repeat_interleave(beam_size, dim=0).contiguous()
        bs = BeamState(B, beam_size, max_len, eos_id, prompt_len=T, device=dev)
        st = GenStateF32(BB, V, 1, dev, pos=bs.pos, next_tok=bs.next_tok)
        rec = torch.empty(max_len, BB, V, dtype=F32, device=dev)
        rec[0].copy_(logits)
        self.beam_step(logits, bs, group_size, diversity_penalty)      # (no reorder: every beam of a prompt still holds its prompt rows only)

        def advance(i, n):
            self.beam_steps(cache, st, bs, group_size, diversity_penalty, rec, n, kv_t0=T)
            return n
        beam_steps_until_done(bs, max_len, advance)
        return beam_hand_out(bs, rec, max_len, self.ops.ctx.sync)

    def _prefill_for_generation(self, embeds, attn_mask, max_len, keep_logits, eos_id=None):
        """How greedy and sampling open (as LlamaEngine._prefill_for_generation): the capacity check, a cache, the state, the prompts
        prefilled, their last-row logits in st.logits, pos = T, step = 0."""
        B, T, _ = embeds.shape
        cache = self.new_cache(B, self._generation_capacity(T, max_len, max_len))
        st = GenStateF32(B, self.cfg.vocab, max_len, self.device, keep_logits, eos_id=eos_id)
        logits, _ = self.prefill(embeds, attn_mask, "last", cache=cache)
        st.logits.copy_(logits)
        st.set(pos=T, step=0)
        return cache, st

    def generate_greedy(self, embeds, attn_mask, max_len, keep_logits=False, graph=True, stop_on_eos=None):
        """`_generate_sampling(greedy=True)` (model_unified.py:861-921) of an fp32 model entirely on the device: the prefill, one pick on its
        logits, then max_len - 1 x (step + pick) without a host synchronisation (`greedy_steps`).  Returns what `LlamaEngine.generate_greedy`
        returns: (tokens [B, max_len] int64, logprob [B], logits [B, steps_run, V] fp32 | None, (state, cache)).
        stop_on_eos (None | eos_id): as in `LlamaEngine.generate_greedy` -- chunks of engine.STOP_CHUNK steps, one look at
        `done` per chunk, at most 2 * STOP_CHUNK - 1 decode steps behind the finishing one; steps_run == max_len without a stop."""
        eos = check_stop_arg(stop_on_eos, self.cfg.vocab, "generate_greedy")
        cache, st = self._prefill_for_generation(embeds, attn_mask, max_len, keep_logits, eos)
        return self.greedy_from_logits(cache, st, embeds.shape[0], max_len, graph=graph) + ((st, cache),)

    def greedy_from_logits(self, cache: KVCacheF32, st: GenStateF32, B, max_len, graph=True):
        """the greedy loop behind a prefill -- st.logits holds its last-row logits, *st.pos the prompt length, *st.step 0: the pick on them,
        max_len - 1 x (step + pick), all at once or, with the state's EOS stop, in chunks, a synchronisation (engine.run_generation) ->
        (tokens [B, max_len] int64, logprob [B], logits [B, steps_run, V] | None).  The one driver of `generate_greedy` and of the model's
        decode_f32="stream" / "device" greedy path."""
        return run_generation(st, max_len, lambda: self.greedy_pick(cache, st, B, advance_pos=False),
                              lambda n: self.greedy_steps(cache, st, B, n, graph=graph), self.ops.ctx.sync)

    def generate_sampling(self, embeds, attn_mask, max_len, temperature=1.0, nucleus_prob=None, keep_logits=False, uniforms=None, graph=True,
                          stop_on_eos=None):
        """`_generate_sampling(greedy=False)` (model_unified.py:861-921) of an fp32 model entirely on the device: the prefill, one pick on its
        logits, then max_len - 1 x (step + pick) without a host synchronisation (`sample_steps`).  The uniform variates of all steps come
        from ONE `torch.rand` on the device generator unless `uniforms` [max_len * B] injects them.  Returns what
        `LlamaEngine.generate_sampling` returns: (tokens [B, max_len] int64, logprob [B], logits [B, max_len, V] fp32 | None, (state, cache,
        variates)).  ValueError before any decode step when max_len tokens do not fit the cache.
        stop_on_eos (None | eos_id): as in `generate_greedy`; the variates keep their positions uniforms[step * B + b]."""
        B = embeds.shape[0]
        eos = check_stop_arg(stop_on_eos, self.cfg.vocab, "generate_sampling")
        u = sampling_variates(uniforms, max_len, B, self.device)
        cache, st = self._prefill_for_generation(embeds, attn_mask, max_len, keep_logits, eos)
        return run_generation(st, max_len, lambda: self.sample_pick(cache, st, B, False, u, temperature, nucleus_prob),
                              lambda n: self.sample_steps(cache, st, B, n, u, temperature, nucleus_prob, graph=graph),
                              self.ops.ctx.sync) + ((st, cache, u),)

    def _rows(self, spec, B, T):
        """flat token rows b*T+t (int64, on the device) of a logit_rows argument: "last", "all", None or a tensor"""
        if isinstance(spec, str) and spec == "last":
            return (torch.arange(B, dtype=torch.int64, device=self.device) + 1) * T - 1
        if isinstance(spec, str) and spec == "all":
            return torch.arange(B * T, dtype=torch.int64, device=self.device)
        if spec is None:
            return torch.zeros(0, dtype=torch.int64, device=self.device)
        if isinstance(spec, str):
            raise ValueError(f'logit_rows={spec!r}: expected "all", "last", None or a tensor of flat rows')
        return spec.to(self.device, torch.int64)

    def _logits(self, hn, rows):
        logits = torch.empty(rows.numel(), self.cfg.vocab, dtype=F32, device=self.device)
        if rows.numel():
            self.ops.linear(hn.index_select(0, rows).contiguous(), self.lm_head, out=logits)
        return logits

    def _mlp(self, x, lw):
        ops, cfg = self.ops, self.cfg
        xn = ops.rmsnorm(x, lw["ln2"], cfg.rms_eps)
        act = ops.silu_mul(ops.linear(xn, lw["wg"]), ops.linear(xn, lw["wu"]))
        return ops.linear(act, lw["wd"], resid=x)

    def _trunk(self, embeds, attn_mask, sum_rows=None, cache=None):
        """the decoder over a whole batch -> (final-normed hidden [B*T, d], sum over the L+1 hidden states at `sum_rows` | None)"""
        ops, cfg = self.ops, self.cfg
        B, T, d = embeds.shape
        _no_shared_prefix(cache)
        if T > cfg.max_pos:
            raise ValueError(f"T={T} exceeds the rotary table ({cfg.max_pos})")
        H, Hkv, dh = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        x = embeds.to(self.device, F32).reshape(B * T, d).contiguous().clone()
        pos = torch.arange(T, dtype=torch.int32, device=self.device).repeat(B)
        cu = torch.arange(B + 1, dtype=torch.int32, device=self.device) * T
        keep = None
        if attn_mask is not None and not bool((attn_mask != 0).all()):
            keep = (attn_mask != 0).to(self.device, torch.uint8).reshape(-1).contiguous()
        srows = None if sum_rows is None else sum_rows.to(self.device, torch.int32).contiguous()
        hsum = None
        if srows is not None:
            hsum = torch.zeros(srows.numel(), d, dtype=F32, device=self.device)
        qw, kw = H * dh, Hkv * dh
        for li, lw in enumerate(self.layers):
            if hsum is not None:
                ops.acc_rows(hsum, x, srows)
            xn = ops.rmsnorm(x, lw["ln1"], cfg.rms_eps)
            qkv = ops.linear(xn, lw["wqkv"])
            ops.rope(qkv, 0, H, dh, pos, self.cos, self.sin)
            ops.rope(qkv, qw, Hkv, dh, pos, self.cos, self.sin)
            if cache is not None:
                cache.k[li, :B, :T] = qkv[:, qw:qw + kw].view(B, T, kw)
                cache.v[li, :B, :T] = qkv[:, qw + kw:].view(B, T, kw)
            ao = ops.attention(qkv, 0, qkv, qw, qkv, qw + kw, cu, keep, B, T, H, Hkv, dh, True, dh ** -0.5)
            x = ops.linear(ao, lw["wo"], resid=x)
            x = self._mlp(x, lw)
        hn = ops.rmsnorm(x, self.final_norm, cfg.rms_eps)
        if hsum is not None:
            ops.acc_rows(hsum, hn, srows)
        return hn, hsum

    def prefill(self, embeds, attn_mask=None, logit_rows="last", want_hidden=False, sum_rows=None, cache=None):
        """embeds [B,T,d] fp32; attn_mask [B,T] 0/1 or None -> (logits [n,V] fp32, final-normed hidden [B,T,d] | None[, sum over the
        L+1 hidden states at `sum_rows` (flat b*T+t) [n,d]]) -- the return contract of `LlamaEngine.prefill`"""
        B, T, d = embeds.shape
        hn, hsum = self._trunk(embeds, attn_mask, sum_rows, cache)
        logits = self._logits(hn, self._rows(logit_rows, B, T))
        hidden = hn.view(B, T, d) if want_hidden else None
        if sum_rows is not None:
            return logits, hidden, hsum
        return logits, hidden

    def _score_rows(self, hn, labels, B, T):
        """HF's shifted causal-LM loss over the rows of hn [B*T, d] (engine.score_plan) -> (token_nll [B,T] fp32, n_tokens): the scored rows
        of the final-normed hidden state are gathered and go through the fused lm_head x cross-entropy; no [n, V] logits"""
        rows_c, tg_c, bt = labels
        n = int(rows_c.numel())
        token_nll = torch.zeros(B, T, dtype=F32, device=self.device)
        if n:
            rows_d, tg_d, bt_d = _h2d_many([rows_c, tg_c, bt.to(torch.int32)], self.device)
            nll = self.ops.lm_head_xent(hn.index_select(0, rows_d.long()).contiguous(), self.lm_head, tg_d)
            token_nll[bt_d[:, 0].long(), bt_d[:, 1].long() + 1] = nll      # row (b, t) scores the token at t + 1
        return token_nll, n

    def score(self, embeds, attn_mask, full_labels, cache=None, logit_rows=None):
        """Teacher-forced scoring in ONE prefill pass, the return contract of `LlamaEngine.score`: embeds [B,T,d] fp32, attn_mask [B,T] or None,
        full_labels [B,>=T] (HF's `labels`: -100 = not scored; a label outside [0, V) is a ValueError) -> (token_nll [B,T] fp32, n_tokens,
        logits | None).  token_nll[b, t+1] = -log p(token t+1 | tokens <= t) where full_labels[b, t+1] is a label, 0 elsewhere; logits [n,V]
        for `logit_rows` (the bits of `prefill`) or None.  Nothing is launched when there is nothing to do."""
        B, T, _ = embeds.shape
        plan = score_plan(full_labels, T, self.cfg.vocab)
        if plan[0].numel() == 0 and logit_rows is None:
            return torch.zeros(B, T, dtype=F32, device=self.device), 0, None
        hn, _ = self._trunk(embeds, attn_mask, None, cache)
        logits = self._logits(hn, self._rows(logit_rows, B, T)) if logit_rows is not None else None
        token_nll, n = self._score_rows(hn, plan, B, T)
        return token_nll, n, logits

    def extend(self, cache: KVCacheF32, embeds, t_past, keep=None, logit_rows=None, labels=None, want_hidden=False, cache_rows=None):
        """S more tokens per row against a cache that holds t_past tokens (HF's forward(inputs_embeds [B,S], past_key_values)), the return tuple of
        `LlamaEngine.extend`: embeds [B,S,d] fp32 at rotary positions t_past .. t_past+S-1 for every row; keep [B, >= t_past+S] (0 = masked key,
        old and new alike) or None; logit_rows "all" / "last" / flat rows b*S+s / None; labels [B,S] in HF's convention (-100 = not scored).
        cache_rows None: the cache is the rows' own -- row b attends its slots [0, t_past) and the new K / V are written to [t_past, t_past+S).
        cache_rows [B]: row b attends slots [0, t_past) of cache row cache_rows[b] (a shared prefix) and nothing is written.
        -> (logits [n,V] | None, hidden [B,S,d] | None, token_nll [B,S] fp32 | None, n_tokens)"""
        ops, cfg = self.ops, self.cfg
        B, S, d = embeds.shape
        t_past = int(t_past)
        _no_shared_prefix(cache)
        if t_past < 0 or t_past > cache.Tmax or (cache_rows is None and (t_past + S > cache.Tmax or B > cache.B)):
            raise ValueError(f"KV cache capacity ({cache.B} rows x {cache.Tmax} slots) exhausted by {B} rows x ({t_past} + {S}) tokens; raise max_new_tokens")
        if t_past + S > cfg.max_pos:
            raise ValueError(f"t_past + S = {t_past + S} exceeds the rotary table ({cfg.max_pos})")
        plan = None if labels is None else score_plan(labels, S, cfg.vocab)
        H, Hkv, dh = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
        keep_d = None
        if keep is not None:
            kp = torch.as_tensor(keep) != 0
            if kp.dim() != 2 or kp.shape[0] != B or kp.shape[1] < t_past + S:
                raise ValueError(f"keep {tuple(kp.shape)}: expected [{B}, >= {t_past + S}]")
            if not bool(kp[:, :t_past + S].all()):
                keep_d = kp[:, :t_past + S].to(self.device, torch.uint8).contiguous()
        crows = None
        if cache_rows is not None:
            cr = torch.as_tensor(cache_rows).reshape(-1).cpu()
            if cr.numel() != B or int(cr.min()) < 0 or int(cr.max()) >= cache.B:
                raise ValueError(f"cache_rows: expected {B} rows of a cache of {cache.B}")
            crows, = _h2d_many([cr.to(torch.int32)], self.device)
        x = embeds.to(self.device, F32).reshape(B * S, d).contiguous().clone()
        pos = (torch.arange(S, dtype=torch.int32, device=self.device) + t_past).repeat(B)
        qw, kw = H * dh, Hkv * dh
        for li, lw in enumerate(self.layers):
            xn = ops.rmsnorm(x, lw["ln1"], cfg.rms_eps)
            qkv = ops.linear(xn, lw["wqkv"])
            ops.rope(qkv, 0, H, dh, pos, self.cos, self.sin)
            ops.rope(qkv, qw, Hkv, dh, pos, self.cos, self.sin)
            if cache_rows is None:
                cache.k[li, :B, t_past:t_past + S] = qkv[:, qw:qw + kw].view(B, S, kw)
                cache.v[li, :B, t_past:t_past + S] = qkv[:, qw + kw:].view(B, S, kw)
            ao = ops.attn_extend(qkv, S, cache.k[li], cache.v[li], t_past, H, Hkv, dh, dh ** -0.5, keep=keep_d, cache_rows=crows)
            x = ops.linear(ao, lw["wo"], resid=x)
            x = self._mlp(x, lw)
        hn = ops.rmsnorm(x, self.final_norm, cfg.rms_eps)
        logits = self._logits(hn, self._rows(logit_rows, B, S)) if logit_rows is not None else None
        token_nll, n = self._score_rows(hn, plan, B, S) if plan is not None else (None, 0)
        return logits, (hn.view(B, S, d) if want_hidden else None), token_nll, n

    def extend_behind(self, prefix_emb, prefix_mask, suffix_emb, suffix_mask, rows_per_prefix, **what):
        """Prefill P prefixes ONCE and run the R = P * rows_per_prefix rows behind them as ONE `extend` on the prefixes' cache (row r reads
        prefix r // rows_per_prefix; the shared-prefix form of `LlamaEngine.extend_behind`): prefix_emb [P,Tp,d], prefix_mask [P,Tp] with the
        pads on the LEFT or None; suffix_emb [R,S,d], suffix_mask [R,S] (0 on the right pads).  what: logit_rows / labels / want_hidden of
        `extend`.  -> (*what `extend` returns, the prefix cache)"""
        if "groups" in what or "packed" in what:
            raise TypeError("LlamaEngineF32.extend_behind: the fp32 family has the shared-prefix form only (no groups=, no packed=)")
        P, Tp, _ = prefix_emb.shape
        R = suffix_emb.shape[0]
        n = int(rows_per_prefix)
        if n < 1 or R != P * n:
            raise ValueError(f"extend_behind: {R} rows are not {P} prefixes x {n} rows")
        cache = self.new_cache(P, Tp)
        self.prefill(prefix_emb, prefix_mask, logit_rows=None, cache=cache)
        full = bool(torch.as_tensor(suffix_mask).all())
        keep = None if full and prefix_mask is None else uniform_keep(prefix_mask, torch.as_tensor(suffix_mask).long(), Tp)
        return (*self.extend(cache, suffix_emb, Tp, keep=keep, cache_rows=torch.arange(R) // n, **what), cache)
