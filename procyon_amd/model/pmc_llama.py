"""Mirror of `LlamaPostTokenization` (/root/reference/procyon/model/pmc_llama.py:415-596) over the HIP engine."""
from __future__ import annotations

from types import SimpleNamespace

import torch

from ..engine import GenState, KVCache, LlamaConfig, LlamaEngine


class _PastF32:
    """fp32 KV cache handle of an fp32 generation: `.cache` (engine_f32.KVCacheF32), `.t` keys held; `.state` (engine_f32.GenStateF32 or
    None): the device state of the stream step -- when set, the cached one-token steps run `LlamaEngineF32.decode_stream` on it"""

    def __init__(self, cache, t, state=None):
        self.cache, self.t, self.state = cache, t, state


class _Past:
    """past_key_values: indexable [layer][0|1] -> [B,Hkv,t,dh] VIEWS of the engine cache, so the in-place row
    re-indexing the reference's beam search performs (model_unified.py:830-832) acts on the live cache.  The views are
    built on access (a decode loop that never looks at them does not pay 2L tensor slicings per step)."""

    def __init__(self, cache: KVCache, t: int):
        self.cache, self.t = cache, t

    def __len__(self):
        return self.cache.k.shape[0]

    def __getitem__(self, l):
        if isinstance(l, slice):
            return [self[i] for i in range(len(self))[l]]
        if l < 0:
            l += len(self)
        if not 0 <= l < len(self):
            raise IndexError(l)
        return [self.cache.k[l, :, :, :self.t], self.cache.v[l, :, :, :self.t]]

    def __iter__(self):
        return (self[l] for l in range(len(self)))


class _HiddenStates:
    """Lazy stand-in for `outputs.hidden_states`, handed out ONLY when the caller asks for it (`lazy_hidden=True`: the engine-backed
    `UnifiedProCyon`, which reads `hidden_states[-1]` alone -- ret_token_access='last', model_unified.py:556-559).  It keeps the last
    state; any other access (another index, iteration, len()) materialises the whole tuple by running the (deterministic) prefill once
    more with every layer's state written out.  It is NOT a tuple -- `torch.stack(obj, -1)` rejects it -- which is why a caller that
    passes the reference's arguments only (INTEGRATION.md route B: the reference's own `UnifiedProCyon` over this sub-module, whose
    ret_token_access='all' branch does `torch.stack(outputs.hidden_states, dim=-1)`, model_unified.py:563) gets a real tuple."""

    def __init__(self, n, last, materialise):
        self._n, self._last, self._mat, self._all = n, last, materialise, None

    def _full(self):
        if self._all is None:
            self._all = tuple(self._mat())
        return self._all

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, int) and (i == -1 or i == self._n - 1) and self._last is not None:
            return self._last
        return self._full()[i]

    def __iter__(self):
        return iter(self._full())


class CausalLMOutput:
    """What `LlamaPostTokenization.forward` returns: `.logits`, `.past_key_values`, `.hidden_states`, `.hidden_state_sum_rows`, `.loss` (HF's
    CausalLMOutputWithPast as the reference reads it) plus `.token_nll` [B,T] fp32 and `.n_tokens` of the scoring pass behind `.loss`.
    The three scoring attributes are None when there is nothing to score with (`scorer` None); otherwise they come from `scorer()` ->
    (token_nll, n_tokens), run on first access and cached -- or at once, by `forward(compute_loss=True)`, which hands the result in.
    loss = token_nll.sum(1).sum() / n_tokens: HF's mean over all labelled tokens of the batch, NaN when there are none."""

    def __init__(self, logits, past_key_values=None, hidden_states=None, hidden_state_sum_rows=None, scorer=None, scored=None):
        self.logits, self.past_key_values, self.hidden_states = logits, past_key_values, hidden_states
        self.hidden_state_sum_rows = hidden_state_sum_rows
        self._scorer, self._scored = scorer, scored

    def _score(self):
        if self._scored is None and self._scorer is not None:
            self._scored = self._scorer()
            self._scorer = None
        return self._scored

    @property
    def token_nll(self):
        sc = self._score()
        return None if sc is None else sc[0]

    @property
    def n_tokens(self):
        sc = self._score()
        return None if sc is None else sc[1]

    @property
    def loss(self):
        sc = self._score()
        return None if sc is None else sc[0].sum(1).sum() / sc[1]


class LlamaPostTokenization:
    """forward(input_embeds|input_ids, attn_masks, full_labels, past_key_values, use_cache, output_attentions)
    -> object with .logits, .past_key_values, .hidden_states, .loss   (pmc_llama.py:546-596).

    Exactly one of input_embeds / input_ids (:562).  With the reference's arguments only, the returned object is the
    reference's: `.logits` [B,T,V] for every row and `.hidden_states` a real `tuple` of the L+1 [B,T,d] tensors (the wrapper always
    runs its model with `output_hidden_states=True`, pmc_llama.py:575,584) -- embeddings, outputs of layers 0..L-2, final-normed
    output of layer L-1.
    Extensions used by the engine-backed `UnifiedProCyon` (never required):
      * `lazy_hidden=True`: `.hidden_states` is a `_HiddenStates` (the last state only, the rest materialised on access).
      * `logit_positions`: LongTensor [B] -> logits only at those positions ([B,1,V]); the reference always materialises
        [B,T,V] (1 GB per 2048-token row).  None = all rows.
      * `want_hidden=False` skips the final hidden state, `hidden_sum_positions` asks for the sum over all L+1 states at
        given rows only (ret_token_access='all' without the tuple), `output_hidden_states=True` materialises the tuple eagerly.
      * full_labels / loss: with `full_labels` [B,>=T] (HF's `labels`, -100 = ignored) `.loss` is HF's causal-LM loss (shifted, mean over
        the labelled tokens of the batch, NaN when there are none), with `.token_nll` [B,T] fp32 (token_nll[b, t+1] = NLL of token t+1) and
        `.n_tokens` beside it -- computed by `LlamaEngine.score` (lm_head x cross-entropy fused, no [B,T,V] logits).  `compute_loss=True`
        scores in this call (one pass together with the logits when `lazy_hidden=True` and no hidden-state sum is asked for; the hidden
        states then come from a second pass if they are read).  With the default `compute_loss=False` nothing extra runs here: `.loss` is
        computed on first access by a second, deterministic scoring pass (same bits) and cached, so callers that never read it pay nothing.
        The fp32 path (fp32 `input_embeds`) does the same on the fp32 family (`LlamaEngineF32.score`, pcy_f32_lm_head_xent; one pass with
        `compute_loss=True` whenever no hidden-state sum is asked for).  Without `full_labels` and on the one-token cached decode `.loss` stays None.
      * past_key_values with MORE than one new token (HF's `forward(input_ids [B,S], past_key_values=...)`): `input_ids` [B,S] with S > 1, or
        bf16 `input_embeds` [B,S,d] at any S, extend the filled cache by S tokens per row in one pass (`LlamaEngine.extend`): positions
        t .. t+S-1, causal among the new tokens, every cached key attended.  `attn_masks` None or [B, t+S] (cached AND new keys; 0 = masked),
        `full_labels` [B,S] label the NEW tokens (token_nll[b, s+1] = NLL of new token s+1 given everything before it, the cache included),
        `logit_positions` [B] index the new tokens.  Returns `.logits` [B,S,V] (or [B,1,V]), `.past_key_values` of t+S tokens,
        `hidden_states[-1]` when `want_hidden`, `.loss / .token_nll / .n_tokens` as above (in the same pass with `compute_loss=True`).
        `input_ids` [B,1] stays the decode step, bit for bit.  An fp32 past (the past of an fp32 forward) takes `input_ids` [B,S] or fp32
        `input_embeds` [B,S,d] the same way (`LlamaEngineF32.extend`, pcy_f32_attn_extend); fp32 embeds with a bf16 past are an error.
      * output_attentions: not computed.
      * max_new_tokens: KV capacity reserved beyond the prompt when use_cache=True.
    """

    def __init__(self, state_dict, cfg: LlamaConfig, device=None, max_new_tokens=256):
        # fp32 checkpoints keep their fp32 tensors (references, wherever they live) until the caller asks for bf16 -- as the reference's
        # module holds fp32 parameters until `.bfloat16()` -- so that a caller which never does gets fp32 arithmetic (engine_f32)
        self._src_f32 = dict(state_dict) if any(v.dtype == torch.float32 for v in state_dict.values()) else None
        self._engine_f32 = None
        self.engine = LlamaEngine(state_dict, cfg, device)
        self.cfg = cfg
        self.max_new_tokens = max_new_tokens
        self.model = SimpleNamespace(vocab_size=cfg.vocab, config=SimpleNamespace(hidden_size=cfg.d))
        self._state = None

    def eval(self):
        return self

    @property
    def engine_f32(self):
        """the fp32 prefill engine, built on first use from the retained fp32 weights"""
        if self._engine_f32 is None:
            if self._src_f32 is None:
                raise RuntimeError("fp32 arithmetic was asked for, but this text encoder holds no fp32 weights (built from bf16 tensors, or "
                                   ".bfloat16() was called before): load the checkpoint again and do not call .bfloat16()")
            from ..engine_f32 import LlamaEngineF32
            self._engine_f32 = LlamaEngineF32(self._src_f32, self.cfg, self.engine.device)
        return self._engine_f32

    def drop_fp32(self):
        self._src_f32 = self._engine_f32 = None

    def get_input_embeddings(self):
        return self.engine.embed

    def forward(self, input_embeds=None, input_ids=None, attn_masks=None, full_labels=None, past_key_values=None,
                use_cache=False, output_attentions=None, logit_positions=None, want_hidden=True, hidden_sum_positions=None,
                output_hidden_states=False, lazy_hidden=False, compute_loss=False):
        assert (input_embeds is not None) != (input_ids is not None), "Only one of input_embeds or input_ids can be provided"
        if isinstance(past_key_values, _PastF32):      # fp32 generation: the cached decode step, or the many-token extension
            if input_embeds is not None and input_embeds.dtype != torch.float32:
                raise RuntimeError("an fp32 past takes input_ids or fp32 input_embeds")
            if input_embeds is not None or input_ids.shape[1] != 1:
                return self._forward_extend_f32(input_embeds, input_ids, attn_masks, full_labels, past_key_values, logit_positions, want_hidden,
                                                compute_loss)
            cache, t = past_key_values.cache, past_key_values.t
            st = past_key_values.state
            if st is not None:      # the stream step (generate(decode_f32="stream")): token ids and position written on the device, replayed graph
                if t + 1 > cache.Tmax:
                    raise ValueError(f"KV cache capacity {cache.Tmax} exhausted; raise max_new_tokens")
                st.set(pos=t, next_tok=input_ids.view(-1).to(self.engine_f32.device))
                logits = self.engine_f32.decode_stream(cache, st, input_ids.shape[0], graph=True).clone()
                return CausalLMOutput(logits.view(input_ids.shape[0], 1, -1), _PastF32(cache, t + 1, st))
            logits = self.engine_f32.decode(cache, input_ids.view(-1), t)
            return CausalLMOutput(logits.view(input_ids.shape[0], 1, -1), _PastF32(cache, t + 1))
        if input_embeds is not None and input_embeds.dtype == torch.float32:
            return self._forward_f32(input_embeds, attn_masks, past_key_values, use_cache, logit_positions, want_hidden, hidden_sum_positions,
                                     full_labels, compute_loss)
        eng = self.engine
        if past_key_values is None:
            if input_embeds is None:
                input_embeds = eng.embed_tokens(input_ids)
            B, T, _ = input_embeds.shape
            cache = eng.new_cache(B, T + (self.max_new_tokens if use_cache else 0))
            if logit_positions is None:
                rows = torch.arange(B * T, dtype=torch.int32)
            else:
                rows = (torch.arange(B) * T + logit_positions.cpu().long()).to(torch.int32)
            hsum = None
            embeds_dev = input_embeds.to(eng.device)
            L1 = self.cfg.n_layers + 1

            def materialise():      # the whole tuple, from a second (deterministic) pass; the KV cache it fills is a scratch one
                _, hall = eng.prefill_all(embeds_dev, attn_masks, eng.new_cache(B, T), None)
                return [hall[i] for i in range(L1)]

            scorer = scored = None
            if full_labels is not None:
                labels = torch.as_tensor(full_labels)[:, :T]      # columns beyond T are not run (the reference's trailing pads: all -100)
                scorer = lambda: eng.score(embeds_dev, attn_masks, labels)[:2]
            if scorer is not None and compute_loss and lazy_hidden and not output_hidden_states and hidden_sum_positions is None:
                # loss and logits from ONE pass; the final hidden state is not written by it (read: a second pass)
                token_nll, n_tok, logits = eng.score(embeds_dev, attn_masks, labels, cache=cache, logit_rows=rows)
                scored, scorer = (token_nll, n_tok), None
                hs = _HiddenStates(L1, None, materialise)
            elif output_hidden_states or not lazy_hidden:
                logits, hall = eng.prefill_all(embeds_dev, attn_masks, cache, rows)
                hs = tuple(hall[i] for i in range(L1))
                if hidden_sum_positions is not None:
                    flat = hall.view(L1, B * T, -1)[:, hidden_sum_positions.to(eng.device).long()]
                    hsum = flat.float().sum(0).to(hall.dtype)
            elif hidden_sum_positions is not None:
                # ret_token_access='all': sum of all L+1 hidden states, only at the requested flat token rows
                logits, hidden, hsum = eng.prefill(embeds_dev, attn_masks, cache, rows, want_hidden=want_hidden,
                                                   sum_rows=hidden_sum_positions)
                hs = _HiddenStates(L1, hidden, materialise)
            else:
                logits, hidden = eng.prefill(embeds_dev, attn_masks, cache, rows, want_hidden=want_hidden)
                hs = _HiddenStates(L1, hidden, materialise)
            logits = logits.view(B, -1, self.cfg.vocab)
            past = _Past(cache, T) if use_cache else None
            out = CausalLMOutput(logits, past, hs, hsum, scorer=scorer, scored=scored)
            if compute_loss:
                out._score()
            return out
        if input_embeds is not None or input_ids.shape[1] != 1:
            return self._forward_extend(input_embeds, input_ids, attn_masks, full_labels, past_key_values, logit_positions, want_hidden, compute_loss)
        # cached decode: one new token per row, no mask, position = cache length (quirks Q1/Q2)
        cache, t = past_key_values.cache, past_key_values.t
        B = input_ids.shape[0]
        if t + 1 > cache.Tmax:
            raise ValueError(f"KV cache capacity {cache.Tmax} exhausted; raise max_new_tokens")
        if self._state is None or self._state.next_tok.shape[0] != B:
            self._state = GenState(B, self.cfg.vocab, 1, eng.device)
        st = self._state
        st.pos.fill_(t)
        st.next_tok.copy_(input_ids.view(-1).to(torch.int32))
        eng.decode_graph(cache, st, B)
        return CausalLMOutput(st.logits.clone().view(B, 1, -1), _Past(cache, t + 1))

    def _forward_extend(self, input_embeds, input_ids, attn_masks, full_labels, past_key_values, logit_positions, want_hidden, compute_loss):
        """S new tokens per row against the filled cache of `past_key_values` (see the class docstring): one `LlamaEngine.extend` pass"""
        eng = self.engine
        cache, t = past_key_values.cache, past_key_values.t
        if input_embeds is None:
            input_embeds = eng.embed_tokens(input_ids)
        B, S, _ = input_embeds.shape
        if t + S > cache.capacity:
            raise ValueError(f"KV cache capacity {cache.capacity} exhausted; raise max_new_tokens")
        embeds_dev = input_embeds.to(eng.device)
        if attn_masks is not None:
            attn_masks = torch.as_tensor(attn_masks)
            assert tuple(attn_masks.shape) == (B, t + S), f"attn_masks {tuple(attn_masks.shape)}: the cached and the new keys, [{B}, {t + S}]"
        rows = "all" if logit_positions is None else (torch.arange(B) * S + logit_positions.cpu().long()).to(torch.int32)
        labels = None if full_labels is None else torch.as_tensor(full_labels)[:, :S]
        L1 = self.cfg.n_layers + 1

        def no_tuple():
            raise RuntimeError("the cached multi-token forward keeps the final hidden state only (hidden_states[-1])")

        if labels is not None and not compute_loss:
            # `.loss` on first access: the new tokens' K / V are in the cache by then, so the scoring pass rewrites the same slots with the same bits
            logits, hidden, _, _ = eng.extend(cache, embeds_dev, t, keep=attn_masks, logit_rows=rows, want_hidden=want_hidden)
            scorer, scored = (lambda: tuple(eng.extend(cache, embeds_dev, t, keep=attn_masks, labels=labels)[2:])), None
        else:
            logits, hidden, token_nll, n_tok = eng.extend(cache, embeds_dev, t, keep=attn_masks, logit_rows=rows, labels=labels, want_hidden=want_hidden)
            scorer, scored = None, (None if labels is None else (token_nll, n_tok))
        hs = _HiddenStates(L1, hidden, no_tuple) if want_hidden else None
        return CausalLMOutput(logits.view(B, -1, self.cfg.vocab), _Past(cache, t + S), hs, None, scorer=scorer, scored=scored)

    def _forward_f32(self, input_embeds, attn_masks, past_key_values, use_cache, logit_positions, want_hidden, hidden_sum_positions,
                     full_labels=None, compute_loss=False):
        """fp32 embeddings in -> the fp32 prefill (the callers that never call `.bfloat16()`); use_cache=True keeps the K / V rows in an fp32
        cache for the cached decode steps of an fp32 generation (/root/reference/scripts/caption_bulk.py:70-73, 123-132).  With full_labels:
        `.loss` / `.token_nll` / `.n_tokens` from `LlamaEngineF32.score` -- in this pass together with the logits when compute_loss (and no
        hidden-state sum is asked for), else on first access by a second, deterministic pass."""
        if past_key_values is not None:
            raise RuntimeError("fp32 input_embeds take an fp32 past (the past_key_values of an fp32 forward with use_cache=True) or none")
        eng = self.engine_f32
        B, T, _ = input_embeds.shape
        cache = eng.new_cache(B, T + self.max_new_tokens) if use_cache else None
        rows = "all" if logit_positions is None else (torch.arange(B) * T + logit_positions.cpu().long())
        hsum = None
        no_tuple = lambda: (_ for _ in ()).throw(RuntimeError("the fp32 path keeps the final hidden state only (hidden_states[-1])"))
        L1 = self.cfg.n_layers + 1
        scorer = scored = None
        if full_labels is not None:
            labels = torch.as_tensor(full_labels)[:, :T]      # columns beyond T are not run (the reference's trailing pads: all -100)
            scorer = lambda: eng.score(input_embeds, attn_masks, labels)[:2]
        if scorer is not None and compute_loss and hidden_sum_positions is None:
            # loss and logits from ONE pass; the final hidden state comes from a second pass if it is read
            token_nll, n_tok, logits = eng.score(input_embeds, attn_masks, labels, cache=cache, logit_rows=rows)
            scored, scorer = (token_nll, n_tok), None
            hs = _HiddenStates(L1, None, lambda: [None] * (L1 - 1) + [eng.prefill(input_embeds, attn_masks, None, want_hidden=True)[1]])
        elif hidden_sum_positions is not None:
            logits, hidden, hsum = eng.prefill(input_embeds, attn_masks, rows, want_hidden=True, sum_rows=hidden_sum_positions, cache=cache)
            hs = _HiddenStates(L1, hidden, no_tuple)
        else:
            logits, hidden = eng.prefill(input_embeds, attn_masks, rows, want_hidden=True, cache=cache)
            hs = _HiddenStates(L1, hidden, no_tuple)
        out = CausalLMOutput(logits.view(B, -1, self.cfg.vocab), _PastF32(cache, T) if use_cache else None, hs, hsum, scorer=scorer, scored=scored)
        if compute_loss:
            out._score()
        return out

    def _forward_extend_f32(self, input_embeds, input_ids, attn_masks, full_labels, past_key_values, logit_positions, want_hidden, compute_loss):
        """S new tokens per row against the filled fp32 cache of `past_key_values` (see the class docstring): one `LlamaEngineF32.extend` pass"""
        eng = self.engine_f32
        cache, t = past_key_values.cache, past_key_values.t
        if input_embeds is None:
            input_embeds = eng.embed_tokens(input_ids)
        B, S, _ = input_embeds.shape
        if t + S > cache.Tmax:
            raise ValueError(f"KV cache capacity {cache.Tmax} exhausted; raise max_new_tokens")
        if attn_masks is not None:
            attn_masks = torch.as_tensor(attn_masks)
            assert tuple(attn_masks.shape) == (B, t + S), f"attn_masks {tuple(attn_masks.shape)}: the cached and the new keys, [{B}, {t + S}]"
        rows = "all" if logit_positions is None else (torch.arange(B) * S + logit_positions.cpu().long())
        labels = None if full_labels is None else torch.as_tensor(full_labels)[:, :S]

        def no_tuple():
            raise RuntimeError("the cached multi-token forward keeps the final hidden state only (hidden_states[-1])")

        if labels is not None and not compute_loss:
            # `.loss` on first access: the new tokens' K / V are in the cache by then, so the scoring pass rewrites the same slots with the same bits
            logits, hidden, _, _ = eng.extend(cache, input_embeds, t, keep=attn_masks, logit_rows=rows, want_hidden=want_hidden)
            scorer, scored = (lambda: tuple(eng.extend(cache, input_embeds, t, keep=attn_masks, labels=labels)[2:])), None
        else:
            logits, hidden, token_nll, n_tok = eng.extend(cache, input_embeds, t, keep=attn_masks, logit_rows=rows, labels=labels, want_hidden=want_hidden)
            scorer, scored = None, (None if labels is None else (token_nll, n_tok))
        hs = _HiddenStates(self.cfg.n_layers + 1, hidden, no_tuple) if want_hidden else None
        return CausalLMOutput(logits.view(B, -1, self.cfg.vocab), _PastF32(cache, t + S), hs, None, scorer=scorer, scored=scored)

    __call__ = forward
