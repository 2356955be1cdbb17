"""Mirror of `UnifiedProCyon`'s inference API (/root/reference/procyon/model/model_unified.py) over the
MI355X engine: `forward` (QA / retrieval), `generate` (greedy / sampling / nucleus / diverse beam),
`forward_sequences`, plus the host-side text preparation that sits between them and the kernels.

Same method names, argument meaning, in-place side effects and exceptions as the reference, so the callers in
SURVEY.md section 8b (scripts/, evaluate/framework/procyon.py, inference/) can switch by import path
(INTEGRATION.md).  Training-only branches (contrastive loss, MLM, LoRA groups, freezing) are out of scope.
"""
from __future__ import annotations

from contextlib import contextmanager
from dataclasses import dataclass
from itertools import chain
from types import SimpleNamespace
from typing import List, Optional

import torch

from ..engine import BF16, MlpEngine
from .model_utils import left_pad_tensors


@dataclass
class ProCyonConfig:
    """The `ModelArgs` fields that shape the inference path (training_args_IT.py:27-651; shipped values
    configs/llama3-full.yml:29-68)."""
    text_encoder_fname: str = "llama-3-8b"
    use_aaseq_embeddings: bool = False
    protein_pooling_opt: str = "mean"
    protein_pooling_correction_option: bool = False
    long_protein_strategy: str = "split"
    max_protein_len: int = 1024
    max_text_len: int = 2048
    ret_token_access: str = "last"
    roll_num: int = 0
    use_protein_struct: bool = False
    protein_struct_dropout: float = 0.0
    use_drug_embeddings: bool = False
    protein_task_spc_lora: bool = False
    lora_specific_style: str = "none"


def mask_before(full_labels, answer_idx, before_last_answer=False):
    """`mask_before` (model_unified.py:39-60)."""
    answer_found = (full_labels == answer_idx).nonzero()
    if not before_last_answer:
        if torch.any((full_labels == answer_idx).sum(dim=1) > 1):
            raise ValueError('More than one {} token detected in an input'.format(answer_idx))
        found_map = answer_found
    else:
        found_map = torch.tensor([(i, int(answer_found[answer_found[:, 0] == i, 1].max()))
                                  for i in range(full_labels.shape[0])], device=full_labels.device)
    ar = torch.arange(full_labels.shape[1], device=full_labels.device).unsqueeze(0).repeat(full_labels.shape[0], 1)
    ind = found_map[:, 1].unsqueeze(1).repeat(1, full_labels.shape[1])
    return ind >= ar


def multi_replace_tokens(a, b, replace_token, eval=False):
    """`multi_replace_tokens` (model_unified.py:83-108): splice the token lists `b` over the occurrences of
    `replace_token` in `a` ([EXT] slots); eval=True leaves the last slot empty."""
    occ = [i for i, t in enumerate(a) if t == replace_token]
    if len(occ) != len(b):
        raise ValueError("Number of occurrences of replace_token does not match the length of b")
    if len(occ) == 0:
        return a
    result = a[:occ[0]]
    for i, o in enumerate(occ):
        if not (i == len(occ) - 1 and eval):
            result += b[i]
        result += a[o + 1:] if i == len(occ) - 1 else a[o + 1:occ[i + 1]]
    return result


def qa_full_labels(input_ids, pad_id, special_ids, answer_idx, use_llama_tokenizer=False, train_qa_full_lm=False):
    """The labels `forward` scores a QA / caption batch against (model_unified.py:520-546): the ids with -100 on the pads, on the soft-token
    slots (`special_ids`), on the last column (Llama tokenizer) and -- unless train_qa_full_lm -- on everything up to and including the last
    [ANSWER] of the row."""
    full_labels = input_ids.clone()
    all_masks = full_labels == pad_id
    for i in special_ids:
        all_masks |= full_labels == i
    if use_llama_tokenizer:
        all_masks[:, -1] = True
    if not train_qa_full_lm:
        all_masks |= mask_before(full_labels, answer_idx, before_last_answer=True)
    return torch.where(all_masks, -100, full_labels)


def _pad_rows(rows, fill, left=False):
    """a list of 1-D tensors -> [R, the longest] int64, `fill` in the padding: on the right, or on the left"""
    width = max(int(t.numel()) for t in rows)
    out = torch.full((len(rows), width), int(fill), dtype=torch.long)
    for r, t in enumerate(rows):
        lo = width - int(t.numel()) if left else 0
        out[r, lo:lo + int(t.numel())] = t
    return out


def _pad_mask(rows, left=False):
    """the mask that goes with `_pad_rows(rows, ..., left)`: 1 on the tokens, 0 on the padding"""
    return _pad_rows([torch.ones_like(t) for t in rows], 0, left)


def _cut_candidates(tokenize, label_rule, instructions, candidates, answer_idx, pad_id):
    """What both candidate planners share (arguments as `candidate_plan`; lists of any lengths >= 1): the texts, their tokens and labels,
    and every row cut IN FRONT of its last [ANSWER].  -> (owner, prefixes, suffix):
      owner[r] = (p, n)   row r is candidate n of prompt p, prompt after prompt
      prefixes[p]         the tokens in front of the cut, identical for the rows of a prompt
      suffix              dict: suffix_ids / suffix_mask / suffix_labels [R, S], the rows behind the cut RIGHT-padded with pad_id / 0 / -100; cut [R]
    Every ValueError of the planners' docstrings but the ones on the shape of the lists and on an empty prefix."""
    P = len(instructions)
    if len(candidates) != P or P == 0:
        raise ValueError(f"{len(candidates)} candidate lists for {P} prompts")
    if any(len(c) < 1 for c in candidates):
        raise ValueError(f"every prompt needs at least one candidate, got {[len(c) for c in candidates]}")
    owner = [(p, n) for p in range(P) for n in range(len(candidates[p]))]
    texts = [instructions[p] + " " + candidates[p][n] for p, n in owner]
    ids, mask = tokenize(texts)
    ids, mask = torch.as_tensor(ids).long().cpu(), torch.as_tensor(mask).cpu() != 0
    for r in range(len(owner)):      # (before the label rule, which has no answer for such a row)
        if not bool(((ids[r] == answer_idx) & mask[r]).any()):
            raise ValueError(f"row {r}: no [ANSWER] token in {texts[r]!r}")
    labels = torch.as_tensor(label_rule(ids)).long().cpu()
    prefixes, suffixes, suf_labels, cuts = [], [], [], []
    for r, (p, n) in enumerate(owner):
        n_real = int(mask[r].sum())
        assert bool(mask[r, :n_real].all()), "rows must be right-padded"
        cut = int((ids[r, :n_real] == answer_idx).nonzero().max())
        if bool((labels[r, :cut + 1] != -100).any()):
            raise ValueError(f"row {r}: labelled tokens in front of the last [ANSWER]; they lie in the shared prefix and cannot be scored by the extension")
        if n == 0:
            prefixes.append(ids[r, :cut])
        elif not torch.equal(prefixes[-1], ids[r, :cut]):
            raise ValueError(f"prompt {p}: candidate {n} changes the tokens in front of [ANSWER]; the candidates of a prompt must share its prefix")
        cuts.append(cut)
        suffixes.append(ids[r, cut:n_real])
        suf_labels.append(labels[r, cut:n_real])
    return owner, prefixes, dict(suffix_ids=_pad_rows(suffixes, pad_id), suffix_mask=_pad_mask(suffixes),
                                 suffix_labels=_pad_rows(suf_labels, -100), cut=torch.tensor(cuts))


def candidate_plan(tokenize, label_rule, instructions, candidates, answer_idx, pad_id):
    """Host side of `UnifiedProCyon.score_candidates`: P prompts (instructions ending in [ANSWER]) x N candidate texts each, cut into the part
    all candidates of a prompt share and the part that differs.  Pure: no device, no model.
      tokenize(texts)  -> (ids [R, T], mask [R, T]) right-padded rows, eos included (`_prepare_text_inputs_and_tokenize(texts, [[]] * R, crop_off=True)`)
      label_rule(ids)  -> labels [R, T], the rule `forward` applies to `full_labels` (`qa_full_labels`)
    Row p*N + n is `instructions[p] + " " + candidates[p][n]`, tokenised exactly as `score_text` would, and cut IN FRONT of its last [ANSWER]:
    the prefix (identical for the N rows of a prompt -- ValueError otherwise) and the suffix [ANSWER] + candidate + eos, which holds every
    scored token.  -> dict:
      prefix_ids / prefix_mask [P, Tp]   the prefixes LEFT-padded to the longest (as `generate` pads its prompts), mask 0 on the pads
      suffix_ids / suffix_mask [P*N, S]  the suffixes RIGHT-padded to the longest
      suffix_labels [P*N, S]             the labels of the suffix tokens, -100 on [ANSWER] and on the pads (HF's convention: `extend` shifts)
      n_tokens [P, N]                    scored tokens per row = what `forward`'s rule gives for the concatenated row
      cut [P*N], P, N, Tp, S
    ValueError: candidate lists of unequal length (ragged lists are out of scope), no candidates, a row without [ANSWER], candidates of a
    prompt whose prefixes differ, or labels in front of the cut (train_qa_full_lm: those rows lie in the prefix and cannot be scored here)."""
    counts = [len(c) for c in candidates]
    if len(counts) == len(instructions) > 0 and (counts[0] == 0 or len(set(counts)) > 1):     # (any other count of lists: the cutter's error)
        raise ValueError(f"every prompt needs the same number of candidates, got {counts}")
    _, prefixes, suffix = _cut_candidates(tokenize, label_rule, instructions, candidates, answer_idx, pad_id)
    P, N, Tp = len(prefixes), counts[0], max(int(t.numel()) for t in prefixes)
    if Tp == 0:
        raise ValueError("[ANSWER] is the first token of a row: nothing to prefill")
    return dict(prefix_ids=_pad_rows(prefixes, pad_id, left=True), prefix_mask=_pad_mask(prefixes, left=True),
                **suffix, n_tokens=(suffix["suffix_labels"][:, 1:] != -100).sum(1).view(P, N), P=P, N=N, Tp=Tp, S=suffix["suffix_ids"].shape[1])


def _qa_batch_view(ids, mask, slot_sources, answer_idx, soft_slot_ids):
    """The validated view of a QA batch that both shared-prefix planners cut (their arguments, their ValueErrors) -> (ids [B, T] int64,
    mask [B, T] bool, is_slot [B, T] bool: the real soft-token slots, answer_pos: the column of every row's LAST [ANSWER] among its real tokens)"""
    ids, mask = torch.as_tensor(ids).long().cpu(), torch.as_tensor(mask).cpu() != 0
    if ids.dim() != 2 or ids.shape != mask.shape or ids.shape[0] == 0:
        raise ValueError(f"ids {tuple(ids.shape)} / mask {tuple(mask.shape)}: expected two equal [B, T] arrays, B >= 1")
    B, T = ids.shape
    if len(slot_sources) != B:
        raise ValueError(f"{len(slot_sources)} slot source lists for {B} rows")
    right_padded = torch.arange(T)[None] < mask.sum(1)[:, None]
    if not bool((mask == right_padded).all()):
        raise ValueError(f"row {int((mask != right_padded).any(1).nonzero()[0])} is not right-padded")
    is_ans = (ids == int(answer_idx)) & mask
    if not bool(is_ans.any(1).all()):
        raise ValueError(f"row {int((~is_ans.any(1)).nonzero()[0])}: no [ANSWER] token")
    is_slot = torch.zeros_like(mask)
    for i in soft_slot_ids:
        is_slot |= ids == int(i)
    is_slot &= mask
    for r, n in enumerate(is_slot.sum(1).tolist()):
        if n != len(slot_sources[r]):
            raise ValueError(f"row {r}: {n} soft-token slots, {len(slot_sources[r])} sources")
    return ids, mask, is_slot, (T - 1 - is_ans.flip(1).int().argmax(1)).tolist()


def _shared_cut(ids, mask, is_slot, slot_sources, answer_pos):
    """Tp of `shared_prefix_plan` for the rows of a `_qa_batch_view` (or of a subset of them)"""
    # columns in front of the first one that differs between the rows (or is a pad somewhere), at most the earliest answer position ...
    same = ((ids == ids[0:1]) & mask).all(0)
    Tp = min(min(answer_pos), ids.shape[1] if bool(same.all()) else int((~same).int().argmax()))
    # ... and in front of the first soft slot whose sources differ (the columns up to there are identical: slot k sits at the same column)
    for k, c in enumerate(is_slot[0, :Tp].nonzero()[:, 0].tolist()):
        if any(src[k] != slot_sources[0][k] for src in slot_sources[1:]):
            return c
    return Tp


def shared_prefix_plan(ids, mask, slot_sources, answer_idx, soft_slot_ids, pad_id):
    """Host side of `UnifiedProCyon.forward(share_prefix=True)`: where a QA batch can be cut into the part every row shares and the part
    that differs.  Pure: no device, no model.
      ids / mask [B, T]   the right-padded rows `forward` tokenises (mask 0 on the pads)
      slot_sources[i]     in row order, what feeds each soft-token slot of row i (a token of `soft_slot_ids`): any comparable value per
                          slot, e.g. ("seq", inputs["input"]["seq"][i][k]) -- two slots hold the same embedding iff their sources are equal
    Tp is the largest t such that columns [0, t) are real and identical in every row, the soft slots inside them have equal sources, and
    t <= min_i(position of the last [ANSWER] of row i): every answer row lies in the suffix, S >= 1.  -> dict:
      Tp, S, B
      suffix_ids / suffix_mask [B, S]   tokens [Tp, answer_pos_i] of every row (the answer token included, what follows it is not needed
                                        for the answer logits), right-padded with pad_id / 0
      answer_pos [B]                    position of the last [ANSWER] in the full row
      answer_rows [B] int32             flat row b * S + answer_pos_b - Tp of the [B, S] suffix batch
    ValueError: a row without [ANSWER], rows that are not right-padded, slot_sources that do not match the slots of a row."""
    ids, mask, is_slot, answer_pos = _qa_batch_view(ids, mask, slot_sources, answer_idx, soft_slot_ids)
    B = ids.shape[0]
    Tp = _shared_cut(ids, mask, is_slot, slot_sources, answer_pos)
    suffixes = [ids[r, Tp:answer_pos[r] + 1] for r in range(B)]
    S = max(answer_pos) - Tp + 1
    ap = torch.tensor(answer_pos, dtype=torch.long)
    return dict(Tp=Tp, S=S, B=B, suffix_ids=_pad_rows(suffixes, pad_id), suffix_mask=_pad_mask(suffixes),
                answer_pos=ap, answer_rows=(torch.arange(B) * S + ap - Tp).to(torch.int32))


def shared_prefix_groups(ids, mask, slot_sources, answer_idx, soft_slot_ids, pad_id):
    """Host side of `UnifiedProCyon.forward(share_prefix="groups")`: a QA batch that mixes several shared prefixes (receptors), cut into
    GROUPS of rows with a prefix each.  Pure: no device, no model.  Arguments as `shared_prefix_plan`.
      key     of a row: its real tokens in front of its last soft-token slot in front of its last [ANSWER] (in front of the [ANSWER] if no
              slot lies there), soft slots compared by their source
      groups  rows with equal keys, numbered in order of first appearance
      cut     within a group exactly what `shared_prefix_plan` returns for the group's rows: a one-group batch reproduces that plan
    -> dict:
      order [B] / inverse [B]          rows sorted by group (stable): sorted row i is caller row order[i]; inverse[order[i]] == i
      group_rows / group_len [n]       rows per group; the group's Tp (0 = the group shares nothing: there is no grouped call for such a batch)
      prefix_rows [n]                  the first caller row of every group: its columns [0, group_len[g]) are the group's prefix
      prefix_T, S, B, n_groups         max(group_len); the longest suffix over all groups
      suffix_ids / suffix_mask [B, S]  in SORTED order: tokens [group_len[g], answer_pos] of every row, right-padded with pad_id / 0
      answer_pos [B]                   caller order, position in the full row
      answer_rows [B] int32            flat row i * S + answer_pos - group_len[g] of the sorted [B, S] suffix batch
    ValueError: as `shared_prefix_plan`."""
    ids, mask, is_slot, answer_pos = _qa_batch_view(ids, mask, slot_sources, answer_idx, soft_slot_ids)
    B = ids.shape[0]
    id_rows, slot_rows = ids.tolist(), is_slot.tolist()
    groups, members = {}, []
    for r in range(B):
        slot_cols = [c for c, f in enumerate(slot_rows[r]) if f]
        front = [c for c in slot_cols if c < answer_pos[r]]
        end = front[-1] if front else answer_pos[r]
        row = id_rows[r][:end]
        for c, src in zip(slot_cols, slot_sources[r]):            # a slot is what feeds it, not its token
            if c < end:
                row[c] = ("slot", src)
        key = tuple(row)
        if key not in groups:
            groups[key] = len(members)
            members.append([])
        members[groups[key]].append(r)
    order = [r for rows in members for r in rows]
    inverse = [0] * B
    for i, r in enumerate(order):
        inverse[r] = i
    group_len = [_shared_cut(ids[rows], mask[rows], is_slot[rows], [slot_sources[r] for r in rows], [answer_pos[r] for r in rows]) for rows in members]
    row_len = [n for n, rows in zip(group_len, members) for _ in rows]                   # sorted order, as everything per row below
    suffixes = [ids[r, n:answer_pos[r] + 1] for r, n in zip(order, row_len)]
    suffix_ids = _pad_rows(suffixes, pad_id)
    S = suffix_ids.shape[1]
    ap = torch.tensor(answer_pos, dtype=torch.long)
    return dict(order=torch.tensor(order), inverse=torch.tensor(inverse), group_rows=[len(rows) for rows in members], group_len=group_len,
                prefix_rows=[rows[0] for rows in members], prefix_T=max(group_len), S=S, B=B, n_groups=len(members), suffix_ids=suffix_ids,
                suffix_mask=_pad_mask(suffixes), answer_pos=ap,
                answer_rows=(torch.arange(B) * S + ap[order] - torch.tensor(row_len)).to(torch.int32))


def candidate_plan_groups(tokenize, label_rule, instructions, candidates, answer_idx, pad_id):
    """`candidate_plan` for RAGGED candidate lists (`score_candidates(ragged=True)`): P prompts with len(candidates[p]) >= 1 texts each.  The
    rows are cut as there (in front of the last [ANSWER]; same ValueErrors but the one on unequal lists), prompt after prompt; what differs:
      prefix_ids / prefix_mask [P, Tp]   the prefixes RIGHT-padded: every prompt starts at position 0, where `score_text` has it
      group_rows / group_len [P]         candidates per prompt; real tokens of every prefix -- the tables of `LlamaEngine.new_grouped_cache`
      suffix_ids / suffix_mask / suffix_labels [R, S], cut [R]   R = sum(group_rows) rows
      n_candidates [P], row_of [P, Nmax] the row of candidate (p, n), -1 in the padding; n_tokens [P, Nmax], 0 in the padding
      P, Nmax, R, Tp, S"""
    owner, prefixes, suffix = _cut_candidates(tokenize, label_rule, instructions, candidates, answer_idx, pad_id)
    group_len = [int(t.numel()) for t in prefixes]
    if min(group_len) == 0:
        raise ValueError("[ANSWER] is the first token of a row: nothing to prefill")
    n_cand = [len(c) for c in candidates]
    P, Nmax, R = len(prefixes), max(n_cand), len(owner)
    at = tuple(torch.tensor(owner).T)                                            # (p, n) of every row
    row_of = torch.full((P, Nmax), -1, dtype=torch.long)
    row_of[at] = torch.arange(R)
    n_tokens = torch.zeros(P, Nmax, dtype=torch.long)
    n_tokens[at] = (suffix["suffix_labels"][:, 1:] != -100).sum(1)
    return dict(prefix_ids=_pad_rows(prefixes, pad_id), prefix_mask=_pad_mask(prefixes), group_rows=n_cand,
                group_len=group_len, **suffix, n_candidates=torch.tensor(n_cand), row_of=row_of, n_tokens=n_tokens, P=P, Nmax=Nmax, R=R,
                Tp=max(group_len), S=suffix["suffix_ids"].shape[1])


def special_token_ids(tokenizer, text_encoder_fname):
    """The token ids `UnifiedProCyon.__init__` / `_init_tokenizer` keep (model_unified.py:1100-1133, 342-347), read from a
    tokenizer on which the eight ProCyon tokens are already registered (`procyon_amd.checkpoint.hf_tokenizer` does that in the
    reference's order; the reference reads them back with `tokenizer(tok, add_special_tokens=False).input_ids[0]`, which for an
    added token is its id).  Llama-3 names take the yes / no ids of " yes" / " no" (leading space), others of "yes" / "no"."""
    t = tokenizer
    ids = dict(prot_replacement_idx=t.convert_tokens_to_ids("<|protein|>"), prot_retrieval_idx=t.convert_tokens_to_ids("[PROT]"),
               answer_idx=t.convert_tokens_to_ids("[ANSWER]"), struct_idx=t.convert_tokens_to_ids("<|struct|>"),
               drug_idx=t.convert_tokens_to_ids("<|drug|>"), ext_idx=t.convert_tokens_to_ids("[EXT]"))
    if "llama-3" in text_encoder_fname.lower():  # model_unified.py:342-347
        ids["yes_token"] = t.encode(" yes", add_special_tokens=False)[0]
        ids["no_token"] = t.encode(" no", add_special_tokens=False)[0]
    else:
        ids["yes_token"] = t.encode("yes", add_special_tokens=False)[0]
        ids["no_token"] = t.encode("no", add_special_tokens=False)[0]
    return ids


class _LazyLogits:
    """`outputs.logits` of `UnifiedProCyon.forward` on the QA branch: behaves like the reference's [B, T, V] tensor
    (model_unified.py:548-554) for a caller that indexes it -- `logits[torch.arange(B), pos]`, `logits[:, pos]`, `logits.softmax(-1)`, any
    torch function -- but only the answer rows exist until something else is asked for: indexing exactly the answer positions returns them
    (the QA readers' access, data/inference_utils.py:582-604), anything else runs the prefill once more with every row's logits and caches
    the [B, T_real, V] tensor (columns beyond the last real token of the longest row are never computed; the reference pads to
    max_text_len).  `outputs.answer_logits` [B, 1, V] is the engine's own fast handle on the same rows."""

    def __init__(self, answer_rows, answer_pos, T, materialise):
        self._rows, self._pos, self._T, self._mk, self._full_t = answer_rows, answer_pos.long().cpu(), T, materialise, None

    def _full(self):
        if self._full_t is None:
            self._full_t = self._mk()
        return self._full_t

    @property
    def shape(self):
        return torch.Size((self._rows.shape[0], self._T, self._rows.shape[-1]))

    def size(self, d=None):
        return self.shape if d is None else self.shape[d]

    def dim(self):
        return 3

    @property
    def dtype(self):
        return self._rows.dtype

    @property
    def device(self):
        return self._rows.device

    def _is_answer_index(self, idx):
        if not (isinstance(idx, tuple) and len(idx) == 2):
            return False
        r, p = idx
        B = self._rows.shape[0]
        if isinstance(r, slice):
            if r != slice(None):
                return False
        else:
            r = torch.as_tensor(r).cpu()
            if r.dtype == torch.bool or r.shape != (B,) or not torch.equal(r.long(), torch.arange(B)):
                return False
        if isinstance(p, (int, slice)):
            return False
        p = torch.as_tensor(p).cpu()
        return p.dtype != torch.bool and p.shape == (B,) and torch.equal(p.long(), self._pos) and not isinstance(idx[0], slice)

    def __getitem__(self, idx):
        if self._full_t is None and self._is_answer_index(idx):
            return self._rows
        return self._full()[idx]

    def __getattr__(self, name):      # anything a tensor has (softmax, float, cpu, argmax, ...): on the materialised tensor
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._full(), name)

    def __len__(self):
        return self._rows.shape[0]

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        un = lambda a: a._full() if isinstance(a, _LazyLogits) else a
        return func(*[un(a) for a in args], **{k: un(v) for k, v in (kwargs or {}).items()})


class UnifiedProCyon:
    def __init__(self, config: ProCyonConfig, text_encoder, tokenizer, protein_seq_encoder=None, token_projectors=None,
                 aaseq_shared_projector: Optional[MlpEngine] = None, aaseq_lm_projector: Optional[MlpEngine] = None,
                 protein_seq_embeddings=None, domain_embeddings=None, peptide_embeddings=None,
                 protein_struct_embeddings=None, drug_structure_embeddings=None):
        self.config = config
        self.text_encoder = text_encoder
        self.tokenizer = tokenizer
        self.protein_seq_encoder = protein_seq_encoder
        self.token_projectors = token_projectors or {}
        self.aaseq_shared_projector = aaseq_shared_projector
        self.aaseq_lm_projector = aaseq_lm_projector
        self.protein_seq_embeddings = protein_seq_embeddings
        self.domain_embeddings = domain_embeddings
        self.peptide_embeddings = peptide_embeddings
        self.protein_struct_embeddings = protein_struct_embeddings
        self.drug_structure_embeddings = drug_structure_embeddings
        self.input_embeddings = SimpleNamespace(weight=text_encoder.get_input_embeddings())
        self.device = text_encoder.engine.device
        self.training = False
        self.dtype = torch.float32     # until the caller asks for bf16 (see `bfloat16` below)
        self._tables_f32 = {}          # fp32 embedding tables of an fp32 checkpoint (checkpoint.build_model), kept until .bfloat16()
        self._tables_f32_dev = {}
        self.use_llama_tokenizer = True
        self.train_qa_full_lm = False
        self.struct_dropout_prob = config.protein_struct_dropout
        # special tokens, registered in the order of `_init_tokenizer` (model_unified.py:1100-1133)
        for k, v in special_token_ids(tokenizer, config.text_encoder_fname).items():
            setattr(self, k, v)

    # nn.Module protocol used by the callers (retrieval_utils.py:90-101, procyon.py:64-67).  The reference model is built in the
    # checkpoint's dtype (fp32) and every shipped entry point calls `.bfloat16()` before the first forward -- except
    # examples/paper_analyses/protpep_qa_scores.py:55-58, scripts/qa_filter_captions.py:17-18 and scripts/caption_bulk.py:72-73, which
    # run fp32.  The model tracks the dtype its caller has asked for and computes in it: bf16 on the bf16 engine; fp32 -- as long as the
    # fp32 weights of the checkpoint are still held, i.e. `.bfloat16()` was never called -- on the fp32 operator family
    # (procyon_amd/engine_f32.py: forward, forward_sequences AND generation, `_generate_*_f32`).  Never silently different arithmetic.
    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("training is outside the engine's scope (inference / generation only)")
        return self.eval()

    def bfloat16(self):
        self.dtype = BF16
        # the reference's parameters ARE bf16 from here on: the fp32 copies go (they are 2x the bf16 engine's memory)
        for m in [self.text_encoder, self.protein_seq_encoder, self.aaseq_shared_projector, self.aaseq_lm_projector] + list(self.token_projectors.values()):
            if m is not None and hasattr(m, "drop_fp32"):
                m.drop_fp32()
        self._tables_f32, self._tables_f32_dev = {}, {}
        return self

    @property
    def _f32(self):
        return self.dtype == torch.float32

    def _check_fp32_sources(self):
        # (advisor finding, round 4: after .bfloat16() the fp32 weights are gone; a later .float() must fail HERE, not inside forward)
        enc = self.text_encoder
        if enc is not None and getattr(enc, "_src_f32", None) is None and getattr(enc, "_engine_f32", None) is None:
            raise RuntimeError("UnifiedProCyon.float(): the fp32 weights of this model were dropped by .bfloat16() (or the checkpoint was bf16); "
                               "reload the checkpoint to compute in fp32")

    def float(self):
        self._check_fp32_sources()
        self.dtype = torch.float32
        return self

    def half(self):
        self.dtype = torch.float16
        return self

    def to(self, *args, **kwargs):
        """`nn.Module.to`: a dtype argument is recorded (see `_require_bf16`); a device must be the engine's device."""
        cand = list(args) + [kwargs.get("dtype"), kwargs.get("device")]
        for a in cand:
            if isinstance(a, torch.dtype):
                if not a.is_floating_point:
                    raise TypeError(f"nn.Module.to only accepts floating point dtypes, but got desired dtype={a}")
                if a == torch.float32 and self.dtype != torch.float32:
                    self._check_fp32_sources()
                self.dtype = a
            elif isinstance(a, (str, torch.device, int)) and a is not None:
                dev = torch.device("cuda", a) if isinstance(a, int) else torch.device(a)
                mine = torch.device(self.device)
                if dev.type != mine.type or (dev.index is not None and mine.index is not None and dev.index != mine.index):
                    raise RuntimeError(f"the engine's weights live on {mine}; cannot move the model to {dev} "
                                       "(build it with device=... instead)")
        return self

    def _require_bf16_or_fp32(self, what):
        if self.dtype not in (BF16, torch.float32):
            raise RuntimeError(f"UnifiedProCyon.{what}: the engine computes in bfloat16 or float32, not {self.dtype}")

    def _require_cache_extension(self, what, inputs):
        """what every path over `LlamaEngine.extend` refuses (`forward(share_prefix=...)`, `score_candidates`)"""
        if self._f32:
            raise NotImplementedError(f"{what} needs the bf16 engine (the fp32 family has no cache extension)")
        if self.config.use_protein_struct and inputs["input"]["seq"]:
            raise NotImplementedError(f"{what}: structure tokens are dropped at random per call (struct_dropout_prob), so rows that read alike need "
                                      "not share a prefix; score such batches with the ordinary forward / score_text")
        if bool(self.text_encoder.engine.desc.layers_fp8):
            raise NotImplementedError(f"{what}: the cache extension has no fp8 projections (set_fp8(False) first)")

    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    # ------------------------------------------------------------------------------------------
    def _embed_table(self, aaseq_type):
        tab = {"protein": self.protein_seq_embeddings, "domain": self.domain_embeddings,
               "peptide": self.peptide_embeddings}[aaseq_type]
        if tab is None:
            raise ValueError(f"no embedding table for aaseq_type={aaseq_type}")
        if self._f32:
            return self._table_f32({"protein": "protein_seq_embeddings", "domain": "domain_embeddings", "peptide": "peptide_embeddings"}[aaseq_type])
        return tab

    def _table_f32(self, name):
        if name not in self._tables_f32_dev:
            if name not in self._tables_f32:
                raise RuntimeError(f"fp32 arithmetic was asked for, but the {name} table is held in bf16 only")
            self._tables_f32_dev[name] = self._tables_f32[name].to(self.device, torch.float32)
        return self._tables_f32_dev[name]

    def _encode_aaseq(self, seq, aaseq_type):
        if self.config.use_aaseq_embeddings:
            return self._embed_table(aaseq_type)[seq.to(self.device).long()]
        if self._f32:
            return self.protein_seq_encoder.forward_f32(seq)[0]
        z, _ = self.protein_seq_encoder(seq, aggregate=True)
        return z

    def _full_labels(self, input_ids):
        """the labels `forward` scores against (`qa_full_labels` with this model's token ids)"""
        return qa_full_labels(input_ids, self.tokenizer.pad_token_id, (self.prot_replacement_idx, self.prot_retrieval_idx, self.drug_idx, self.struct_idx),
                              self.answer_idx, self.use_llama_tokenizer, self.train_qa_full_lm)

    def _soft_tokens(self, inputs, aaseq_type):
        """encoder + projector part of `_preprocessing`: (sequence embeddings | None, protein soft tokens | None, drug soft tokens | None)"""
        aaseq_token_embeddings = None
        if inputs["data"]["seq"] is not None:
            aaseq_token_embeddings = self._encode_aaseq(inputs["data"]["seq"], aaseq_type)
        if inputs["input"]["seq"] is not None:
            full_index = list(chain.from_iterable(inputs["input"]["seq"]))
            pz_inputs = aaseq_token_embeddings[torch.tensor(full_index, dtype=torch.long, device=self.device)]
            protein_soft_tokens = self.token_projectors['aaseq'](pz_inputs)
        else:
            protein_soft_tokens = None
        if self.config.use_drug_embeddings and (inputs["data"]["drug"] is not None):
            full_index = list(chain.from_iterable(inputs["input"]["drug"]))
            drug_tab = self._table_f32("drug_structure_embeddings") if self._f32 else self.drug_structure_embeddings
            drug_z = drug_tab[inputs["data"]["drug"].to(self.device).long()][full_index]
            drug_soft_tokens = self.token_projectors["drug"](drug_z)
        else:
            drug_soft_tokens = None
        return aaseq_token_embeddings, protein_soft_tokens, drug_soft_tokens

    def _preprocessing(self, inputs, aaseq_type='protein', exclude_protein_structure=False, crop_off=False,
                       no_pad=False, retrieval=False, left_pad=False):
        """`_preprocessing` (model_unified.py:352-481)."""
        aaseq_token_embeddings, protein_soft_tokens, drug_soft_tokens = self._soft_tokens(inputs, aaseq_type)
        aaseq_ret_embeddings = aaseq_token_embeddings
        text_inputs = [[inputs["data"]["text"][i] for i in inp_list] for inp_list in inputs["input"]["text"]]
        instruction_list = inputs['instructions']
        protein_struct_tokens = []
        if (not exclude_protein_structure) and self.config.use_protein_struct and inputs["input"]["seq"]:
            # mutates inputs["instructions"] in place and draws from the global torch RNG, as the reference
            # does (model_unified.py:422,433-437; quirk Q6)
            include_mask = torch.bernoulli(torch.full((len(instruction_list),), 1 - self.struct_dropout_prob))
            all_row_indices = []
            for i in include_mask.nonzero(as_tuple=True)[0].tolist():
                instruction_list[i] = instruction_list[i].replace("<|protein|>", "<|protein|> <|struct|>")
                all_row_indices.append(torch.cat([inputs["data"]["seq_idx"][j].unsqueeze(0) for j in inputs["input"]["seq"][i]]))
            all_row_indices = torch.stack(all_row_indices, dim=0)
            ari_unique, ari_inverse = all_row_indices.unique(return_inverse=True)
            if aaseq_type == "protein":
                struct_z = (self._table_f32("protein_struct_embeddings") if self._f32 else self.protein_struct_embeddings)[ari_unique.to(self.device).long()]
            else:
                struct_z = torch.zeros(ari_unique.shape[0], self.protein_struct_embeddings.shape[1], dtype=self.dtype, device=self.device)
            token_z_expand = self.token_projectors["prot_structure"](struct_z)[ari_inverse.to(self.device)]
            for i, val in enumerate(include_mask):
                protein_struct_tokens.append(token_z_expand[i, ...] if val else [])
        input_ids, attn_masks = self._prepare_text_inputs_and_tokenize(
            instruction_list, text_inputs, crop_off=crop_off, retrieval=retrieval, no_pad=no_pad, left_pad=left_pad)
        input_embeds, ret_output_indices = self._prepare_input_embeddings(
            input_ids, protein_soft_tokens=protein_soft_tokens, protein_struct_tokens=protein_struct_tokens,
            drug_soft_tokens=drug_soft_tokens)
        return input_embeds, input_ids, attn_masks, ret_output_indices, aaseq_token_embeddings, aaseq_ret_embeddings

    def _prepare_text_inputs_and_tokenize(self, instructions: List[str], text_input_list: List[List[str]], crop_off=False,
                                          retrieval=False, no_pad=False, left_pad=False):
        """`_prepare_text_inputs_and_tokenize` (model_unified.py:1177-1293), eval path (no crop sampling)."""
        tk = self.tokenizer
        assert all([t[-1] != tk.sep_token for t in instructions])
        instruction_tokens = tk(instructions, padding=False, truncation=True, add_special_tokens=True,
                                max_length=self.config.max_text_len)['input_ids']
        max_len = max(len(l) for l in instruction_tokens)
        joint_tokens, attention_masks = [], []
        for i, text_input in enumerate(text_input_list):
            n_txt = len(text_input)
            if n_txt != 0:
                for j in range(n_txt):
                    if not isinstance(text_input[j], str):
                        text_input[j] = "null"
                toks = tk(text_input, padding=False, truncation=False, add_special_tokens=False)['input_ids']
                max_len_for_sample = (self.config.max_text_len - max_len) // n_txt
                for j in range(len(toks)):
                    drug_add = None
                    if self.drug_idx in toks[j]:
                        where_drug = toks[j].index(self.drug_idx) - 3
                        drug_add = toks[j][(where_drug - 3):]
                        toks[j] = toks[j][:(where_drug - 3)]
                    end_i = max_len_for_sample - (len(drug_add) if drug_add is not None else 0)
                    toks[j] = toks[j][0:end_i]
                    if drug_add is not None:
                        toks[j] = toks[j] + drug_add
            else:
                toks = []
            Lt = multi_replace_tokens(list(instruction_tokens[i]), toks, self.ext_idx, eval=False)
            if no_pad:
                Lt = torch.tensor(Lt)
            else:
                Lt = torch.tensor(Lt + [tk.eos_token_id] + [tk.pad_token_id] * max(self.config.max_text_len - len(Lt) - 1, 0))
            joint_tokens.append(Lt)
            attention_masks.append((Lt != tk.pad_token_id).int())
            assert not torch.any(Lt == self.ext_idx), 'ERROR [EXT] found in input'
        if left_pad:
            return left_pad_tensors(joint_tokens, pad_value=tk.pad_token_id)
        return torch.stack(joint_tokens, dim=0), torch.stack(attention_masks, dim=0)

    def _prepare_input_embeddings(self, input_ids, protein_soft_tokens=None, protein_struct_tokens=[], drug_soft_tokens=None):
        """`_prepare_input_embeddings` (model_unified.py:1135-1175): embedding lookup with the soft tokens written
        over the <|protein|> / <|struct|> / <|drug|> rows, in row-major order, by ONE gather kernel."""
        ids = input_ids.long()
        flat = ids.reshape(-1)
        soft_map = torch.full((flat.numel(),), -1, dtype=torch.int32)
        pieces, base = [], 0
        if protein_soft_tokens is not None:
            m = flat == self.prot_replacement_idx
            assert int(m.sum()) == protein_soft_tokens.shape[0]
            soft_map[m] = torch.arange(int(m.sum()), dtype=torch.int32) + base
            pieces.append(protein_soft_tokens)
            base += protein_soft_tokens.shape[0]
        if len(protein_struct_tokens) > 0:
            ms = ids == self.struct_idx
            for i in range(ids.shape[0]):
                n = int(ms[i].sum())
                if n > 0:
                    assert n == protein_struct_tokens[i].shape[0], f"expected: {n} got: {protein_struct_tokens[i].shape[0]}"
                    row = torch.zeros_like(ids, dtype=torch.bool)
                    row[i] = ms[i]
                    soft_map[row.reshape(-1)] = torch.arange(n, dtype=torch.int32) + base
                    pieces.append(protein_struct_tokens[i])
                    base += n
        if drug_soft_tokens is not None:
            m = flat == self.drug_idx
            assert int(m.sum()) == drug_soft_tokens.shape[0], f"expected: {int(m.sum())} got: {drug_soft_tokens.shape[0]}"
            soft_map[m] = torch.arange(int(m.sum()), dtype=torch.int32) + base
            pieces.append(drug_soft_tokens)
        soft = torch.cat(pieces, 0).contiguous() if pieces else None
        eng = self.text_encoder.engine_f32 if self._f32 else self.text_encoder.engine
        z = eng.embed_tokens(ids, soft, soft_map if pieces else None)
        ret = ids == self.prot_retrieval_idx
        if self.config.roll_num != 0:
            ret = ret.roll(self.config.roll_num, 1)
        return z, ret

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, inputs, return_mlm=False, retrieval=False, get_full_labels=False, aaseq_type='protein',
                exclude_protein_structure=False, crop_off=False, output_attentions=False, full_logits=False, compute_loss=False,
                share_prefix=False, packed=True):
        """`forward` (model_unified.py:483-581), inference branches.  QA: `outputs.logits` reads like the reference's [B, T, V] tensor
        (:548-554) -- index it at the answer positions (`logits[torch.arange(B), pos]`, data/inference_utils.py:582-604) and the rows that
        were computed come back; any other access materialises every position once (_LazyLogits).  `outputs.answer_logits` [B, 1, V] and
        out["answer_positions"] are the engine's own handle on the answer rows.  Retrieval: contrastive_out["positive"]["text"] [B, D].
        full_logits=True (not in the reference's signature): outputs.logits is a plain [B, T_real, V] tensor from the start (the reference pads
        every row to max_text_len and materialises [B, 2048, V]; the trailing all-pad columns are not computed here).
        `outputs.loss` (non-retrieval, bf16 and fp32): the reference's causal-LM loss over `full_labels` (trainIT.py reads it for the validation
        loss and perplexity), with `outputs.token_nll` / `outputs.n_tokens` -- computed on first access, or in this pass with compute_loss=True
        (LlamaPostTokenization.forward); None for retrieval.
        share_prefix=True (QA, bf16; not in the reference's signature): the columns every row of the batch shares -- in-context examples, the
        receptor -- are prefilled ONCE and the rows' differing ends run as one `LlamaEngine.extend` call on a cache whose rows share that
        prefix (`shared_prefix_plan`; `packed`: with the packed extension attention, read only here).  Same dictionary, plus
        out["prefix_plan"]; the answer logits differ from the ordinary path's by kernel rounding only; `outputs.logits` / `.loss` /
        `.hidden_states` beyond the answer rows come from the ordinary full pass on first access.  A batch that shares nothing (Tp = 0) takes
        the ordinary path.  Not with retrieval, compute_loss or full_logits (ValueError); not on the fp32 family, with structure tokens
        (dropped at random per call) or with fp8 weights (NotImplementedError).
        share_prefix="groups": the batch may mix SEVERAL shared prefixes (receptors).  `shared_prefix_groups` sorts the rows into groups with a
        prefix each; ONE prefill runs the n_groups prefixes (right-padded to the longest, under the mask) and ONE grouped `extend` runs every
        row's end behind its own group's prefix, at the positions the ordinary pass gives it.  The answer logits come back in the caller's row
        order; out["prefix_plan"] is the groups plan.  Same refusals; a batch with a group that shares nothing takes the ordinary path."""
        if share_prefix not in (False, True, "groups"):
            raise ValueError(f"forward: share_prefix={share_prefix!r} (False, True or \"groups\")")
        if return_mlm:
            raise NotImplementedError("return_mlm is a training path (model_unified.py:505-509)")
        self._require_bf16_or_fp32("forward")
        if share_prefix:
            if retrieval:
                raise ValueError("forward(share_prefix=True): retrieval batches read the [PROT] rows of every prompt; there is no shared-prefix path for them")
            if compute_loss or full_logits:
                raise ValueError("forward(share_prefix=True) computes the answer rows only: compute_loss / full_logits need the ordinary pass")
            self._require_cache_extension("forward(share_prefix=True)", inputs)
        input_embeds, input_ids, attn_masks, ret_idx, tok_emb, ret_emb = self._preprocessing(
            inputs, aaseq_type=aaseq_type, crop_off=crop_off, retrieval=retrieval, exclude_protein_structure=False)
        full_labels = None
        B = input_ids.shape[0]
        # the reference right-pads every row to max_text_len (Q13); causal rows are unaffected by trailing pads,
        # so only the columns up to the last real token are run
        real = int(attn_masks.sum(1).max())
        emb = input_embeds[:, :real].contiguous()
        answer_pos = None
        if not retrieval:
            full_labels = self._full_labels(input_ids)
            answer_pos = torch.tensor([int((input_ids[i] == self.answer_idx).nonzero()[:, 0].max()) for i in range(B)])
        if retrieval and self.config.ret_token_access not in ('last', 'all'):
            raise NotImplementedError("Invalid option {} for ret_token_access".format(self.config.ret_token_access))
        if share_prefix:
            branch = self._forward_prefix_groups if share_prefix == "groups" else self._forward_shared_prefix
            out = branch(inputs, emb, input_ids, attn_masks[:, :real], full_labels, answer_pos, real, get_full_labels, packed)
            if out is not None:
                return out
        sum_all = retrieval and self.config.ret_token_access == 'all'
        ret_rows = ret_idx[:, :real].reshape(-1).nonzero()[:, 0] if sum_all else None   # flat b*T + t, row-major like boolean indexing
        # (labels cropped to the columns that are run: the reference's trailing pad columns are all -100)
        outputs = self.text_encoder(input_embeds=emb, attn_masks=attn_masks[:, :real], full_labels=None if full_labels is None else full_labels[:, :real],
                                    compute_loss=compute_loss and not retrieval,
                                    logit_positions=None if full_logits else (answer_pos if not retrieval else torch.zeros(B, dtype=torch.long)),
                                    want_hidden=retrieval and not sum_all, hidden_sum_positions=ret_rows, lazy_hidden=True)
        if not retrieval and not full_logits:
            # the reference's `outputs.logits` is [B, T, V]; here the answer rows are computed and the rest on first access (_LazyLogits)
            enc, am = self.text_encoder, attn_masks[:, :real]
            outputs.answer_logits = outputs.logits                       # [B, 1, V]
            outputs.logits = _LazyLogits(outputs.answer_logits[:, 0], answer_pos, real,
                                         lambda: enc(input_embeds=emb, attn_masks=am, logit_positions=None, want_hidden=False, lazy_hidden=True).logits)
        out = {'outputs': outputs, 'text_toks': input_ids, 'full_labels': full_labels if get_full_labels else None,
               'contrastive_out': None, 'contrastive_loss': None, 'answer_positions': answer_pos}
        if retrieval:
            if sum_all:   # torch.stack(hidden_states, -1).sum(-1)[ret] (model_unified.py:560-563), computed at the [PROT] rows only
                extracted = outputs.hidden_state_sum_rows
            else:
                hidden = outputs.hidden_states[-1]
                extracted = hidden[ret_idx[:, :real].to(hidden.device)]
            shared_lm = self.aaseq_lm_projector(extracted)
            c = {"positive": {}, "negative": {}}
            if inputs["target"]["text"] is None:
                c["positive"]["text"] = shared_lm
            else:
                c["positive"]["text"] = shared_lm[inputs["target"]["text"]["positive"]]
                if inputs["target"]["text"]["negative"] is not None:
                    raise NotImplementedError
            if inputs["target"]["seq"] is not None:
                shared_plm = self.aaseq_shared_projector(ret_emb)
                c["positive"]["sequence"] = shared_plm[inputs["target"]["seq"]["positive"]]
                if inputs['target']["seq"]["negative"] is not None:
                    raise NotImplementedError
            out['contrastive_out'] = c
        return out

    def _slot_sources(self, inputs, input_ids):
        """per row, in row order, what feeds each soft-token slot (`shared_prefix_plan`): ("seq" | "drug", index into inputs["data"])"""
        seq, drug = inputs["input"].get("seq"), inputs["input"].get("drug")
        out = [[] for _ in range(input_ids.shape[0])]
        # (row, column, kind) of every slot, row-major: the slots of a row in row order
        slots = sorted([(i, t, 0) for i, t in (input_ids == self.prot_replacement_idx).nonzero().tolist()] +
                       [(i, t, 1) for i, t in (input_ids == self.drug_idx).nonzero().tolist()])
        k = [[0, 0] for _ in out]
        for i, _, kind in slots:
            out[i].append(("drug" if kind else "seq", int((drug if kind else seq)[i][k[i][kind]])))
            k[i][kind] += 1
        return out

    def _forward_shared_prefix(self, inputs, emb, input_ids, am, full_labels, answer_pos, real, get_full_labels, packed):
        """the share_prefix=True branch of `forward` behind `_preprocessing` (emb [B, real, d], am [B, real]); None = nothing is shared"""
        plan = shared_prefix_plan(input_ids[:, :real], am, self._slot_sources(inputs, input_ids[:, :real]), self.answer_idx,
                                  (self.prot_replacement_idx, self.drug_idx), self.tokenizer.pad_token_id)
        Tp, S, B = plan["Tp"], plan["S"], plan["B"]
        if Tp == 0:
            return None
        # ONE prefix row for the B rows, no prefix mask (columns behind a row's [ANSWER] inside [Tp, Tp + S): masked as keys, and no answer row
        # attends them anyway); suffixes of one length (the screening batches): no mask at all, the kernel takes its unmasked block path
        logits, *_ = self.text_encoder.engine.extend_behind(emb[0:1, :Tp].contiguous(), None, emb[:, Tp:Tp + S].contiguous(), plan["suffix_mask"],
                                                            rows_per_prefix=B, logit_rows=plan["answer_rows"], packed=bool(packed))
        return self._answer_rows_output(logits, plan, emb, input_ids, am, full_labels, answer_pos, real, get_full_labels)

    def _forward_prefix_groups(self, inputs, emb, input_ids, am, full_labels, answer_pos, real, get_full_labels, packed):
        """the share_prefix="groups" branch of `forward`; None = some group shares nothing (the ordinary path serves the batch)"""
        plan = shared_prefix_groups(input_ids[:, :real], am, self._slot_sources(inputs, input_ids[:, :real]), self.answer_idx,
                                    (self.prot_replacement_idx, self.drug_idx), self.tokenizer.pad_token_id)
        if min(plan["group_len"]) == 0:
            return None
        Tp, S = plan["prefix_T"], plan["S"]
        row_len = torch.tensor(plan["group_len"]).repeat_interleave(torch.tensor(plan["group_rows"]))   # [B] in sorted order
        order = plan["order"].to(emb.device)
        cols = (row_len[:, None] + torch.arange(S)[None]).clamp(max=real - 1).to(emb.device)   # (clamped columns lie behind the row's [ANSWER]: masked)
        # the groups' prefixes RIGHT-padded to the longest: the real tokens start at position 0 (the columns behind a shorter prefix hold its
        # first row's own tokens, masked as keys; their K / V slots are never addressed by the extension)
        logits, *_ = self.text_encoder.engine.extend_behind(emb[plan["prefix_rows"], :Tp].contiguous(), None, emb[order[:, None], cols].contiguous(),
                                                            plan["suffix_mask"], groups=(plan["group_rows"], plan["group_len"]),
                                                            logit_rows=plan["answer_rows"], packed=bool(packed))
        return self._answer_rows_output(logits[plan["inverse"].to(logits.device)], plan, emb, input_ids, am, full_labels, answer_pos, real, get_full_labels)

    def _answer_rows_output(self, logits, plan, emb, input_ids, am, full_labels, answer_pos, real, get_full_labels):
        """what both shared-prefix branches return: the answer logits [B, V] (caller order) with the lazy rest of the ordinary pass"""
        from .pmc_llama import CausalLMOutput, _HiddenStates
        enc = self.text_encoder
        eng = enc.engine
        B = input_ids.shape[0]
        L1, labels = eng.cfg.n_layers + 1, full_labels[:, :real]

        def materialise():
            _, hall = eng.prefill_all(emb, am, eng.new_cache(B, real), None)
            return [hall[i] for i in range(L1)]

        outputs = CausalLMOutput(logits.view(B, 1, -1), None, _HiddenStates(L1, None, materialise), None,
                                 scorer=lambda: eng.score(emb, am, labels)[:2])
        outputs.answer_logits = outputs.logits
        outputs.logits = _LazyLogits(outputs.answer_logits[:, 0], answer_pos, real,
                                     lambda: enc(input_embeds=emb, attn_masks=am, logit_positions=None, want_hidden=False, lazy_hidden=True).logits)
        return {'outputs': outputs, 'text_toks': input_ids, 'full_labels': full_labels if get_full_labels else None,
                'contrastive_out': None, 'contrastive_loss': None, 'answer_positions': answer_pos, 'prefix_plan': plan}

    @torch.no_grad()
    def score_text(self, inputs, aaseq_type='protein', crop_off=True):
        """Teacher-forced likelihood of the text behind [ANSWER] in every row of a QA / caption batch (the reference: `forward` +
        `out['outputs'].loss`, `np.exp(loss)` as perplexity, trainIT.py:1213-1217): caption ranking and perplexity filtering.
        -> {"token_nll" [B, T] fp32 (0 where nothing is labelled), "seq_nll" [B] = its row sums, "n_tokens" [B] labelled tokens per row,
        "loss" = seq_nll.sum() / n_tokens.sum() (HF's batch mean), "perplexity" = exp(loss)}.  One prefill pass, no [B, T, V] logits."""
        out = self.forward(inputs, aaseq_type=aaseq_type, crop_off=crop_off, get_full_labels=True, compute_loss=True)
        o = out['outputs']
        tn = o.token_nll
        n_tok = (out['full_labels'][:, 1:tn.shape[1]] != -100).sum(1)
        loss = o.loss
        return {"token_nll": tn, "seq_nll": tn.sum(1), "n_tokens": n_tok, "loss": loss, "perplexity": torch.exp(loss)}

    @torch.no_grad()
    def score_candidates(self, inputs, candidates, aaseq_type='protein', packed=False, ragged=False):
        """Rank N candidate texts per prompt by teacher-forced likelihood WITHOUT running the prompt N times.  `inputs`: a caption / QA batch as
        `generate` takes it, every instruction ending in [ANSWER]; `candidates`: one list of N strings per prompt (the same N for all,
        ValueError otherwise).  Row (p, n) is scored as `score_text` scores `instructions[p] + " " + candidates[p][n]` -- same tokens, same
        labels -- but the prompts are encoded and prefilled ONCE (P rows, left-padded as `generate` pads them) and the P*N suffixes
        [ANSWER] + candidate + eos run as one `LlamaEngine.extend` call on a cache whose rows share the prompts' K / V (`candidate_plan`).
        -> {"token_nll" [P,N,S] fp32 over the suffix tokens (0 where nothing is labelled), "seq_nll" [P,N], "n_tokens" [P,N], "mean_nll" [P,N] =
        seq_nll / n_tokens, "order" [P,N] = stable argsort of mean_nll, best first, "plan" = the `candidate_plan`, "cache" = the shared cache}.
        packed: the extension runs the packed attention (`LlamaEngine.extend(packed=True)`): same bits.
        ragged=True: lists of any lengths >= 1 (`candidate_plan_groups`).  The prompts are RIGHT-padded -- every prompt sits at the positions
        `score_text` gives it and no pad column runs in front of it -- and the suffixes run as one grouped `extend`.  The results are padded to
        Nmax = the longest list: "n_candidates" [P]; in the padding token_nll = 0, n_tokens = 0, seq_nll = mean_nll = +inf, so that "order"
        (stable argsort) puts it last.
        Not with structure tokens or with fp8 weights (NotImplementedError, the refusals of `forward(share_prefix=True)`).  On an fp32 model the
        suffixes run through `LlamaEngineF32.extend_behind` (the prompts' fp32 cache, read by every row behind it; "cache" is that prefix cache);
        `packed` is accepted and ignored (there is one fp32 attention), ragged=True is NotImplementedError."""
        self._require_bf16_or_fp32("score_candidates")
        if self._f32:       # the fp32 family has the shared-prefix form of the extension only (LlamaEngineF32.extend_behind); one attention: `packed` is not read
            if ragged:
                raise NotImplementedError("score_candidates(ragged=True) needs the bf16 engine (the fp32 family has no grouped cache)")
            if self.config.use_protein_struct and inputs["input"]["seq"]:
                raise NotImplementedError("score_candidates: structure tokens are dropped at random per call (struct_dropout_prob), so rows that read "
                                          "alike need not share a prefix; score such batches with the ordinary forward / score_text")
        else:
            self._require_cache_extension("score_candidates", inputs)
        if any(len(t) for t in inputs["input"]["text"]):
            raise NotImplementedError("score_candidates: [EXT] text slots are not supported; write the text into the instruction")
        tokenize = lambda texts: self._prepare_text_inputs_and_tokenize(texts, [[] for _ in texts], crop_off=True)
        plan = (candidate_plan_groups if ragged else candidate_plan)(tokenize, self._full_labels, list(inputs["instructions"]), candidates,
                                                                     self.answer_idx, self.tokenizer.pad_token_id)
        if any(bool((plan["suffix_ids"] == i).any()) for i in (self.prot_replacement_idx, self.struct_idx, self.drug_idx)):
            raise ValueError("score_candidates: a candidate holds a soft-token slot")
        _, protein_soft_tokens, drug_soft_tokens = self._soft_tokens(inputs, aaseq_type)
        prefix_emb, _ = self._prepare_input_embeddings(plan["prefix_ids"], protein_soft_tokens=protein_soft_tokens, drug_soft_tokens=drug_soft_tokens)
        eng = self.text_encoder.engine_f32 if self._f32 else self.text_encoder.engine
        rows = dict(groups=(plan["group_rows"], plan["group_len"])) if ragged else dict(rows_per_prefix=plan["N"])
        if not self._f32:
            rows["packed"] = bool(packed)
        _, _, row_nll, _, cache = eng.extend_behind(prefix_emb, plan["prefix_mask"], eng.embed_tokens(plan["suffix_ids"]), plan["suffix_mask"],
                                                    labels=plan["suffix_labels"], **rows)
        n_tokens = plan["n_tokens"].to(row_nll.device)
        if not ragged:
            token_nll = row_nll.view(plan["P"], plan["N"], plan["S"])
            seq_nll = token_nll.sum(2)
            mean_nll = seq_nll / n_tokens
        else:                                        # [P, Nmax] with the padding of the shorter lists sorted last
            row_of = plan["row_of"].to(row_nll.device)
            real = row_of >= 0
            token_nll = torch.zeros(plan["P"], plan["Nmax"], plan["S"], dtype=row_nll.dtype, device=row_nll.device)
            token_nll[real] = row_nll[row_of[real]]
            inf = torch.full_like(n_tokens, float("inf"), dtype=row_nll.dtype)
            seq_nll = torch.where(real, token_nll.sum(2), inf)
            mean_nll = torch.where(real, seq_nll / n_tokens, inf)
        out = {"token_nll": token_nll, "seq_nll": seq_nll, "n_tokens": n_tokens, "mean_nll": mean_nll,
               "order": torch.argsort(mean_nll, dim=1, stable=True), "plan": plan, "cache": cache}
        return dict(out, n_candidates=plan["n_candidates"]) if ragged else out

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def from_pretrained(**kw):
        """`UnifiedProCyon.from_pretrained` (model_unified.py:1296-1394); see procyon_amd.checkpoint.from_pretrained."""
        from ..checkpoint import from_pretrained
        return from_pretrained(**kw)

    @staticmethod
    def get_checkpoint_configs(resume_from_checkpoint):
        """(data_args, model_args, train_args) (model_unified.py:1396-1406)"""
        from ..checkpoint import get_checkpoint_configs
        return get_checkpoint_configs(resume_from_checkpoint)

    def forward_sequences(self, seq_input, get_soft_tokens=False, aaseq_type="protein"):
        """`forward_sequences` (model_unified.py:1029-1086)."""
        self._require_bf16_or_fp32("forward_sequences")
        if isinstance(seq_input, dict):
            seq_input = seq_input["data"]
        z = self._encode_aaseq(seq_input, aaseq_type)
        out = {"original": z, "shared": self.aaseq_shared_projector(z), "token": None}
        if get_soft_tokens:
            out["token"] = self.token_projectors['aaseq'](z)
        return out

    # ------------------------------------------------------------------------------------------
    def _get_nucleus_mask(self, probs, nucleus_prob):
        """`_get_nucleus_mask` (model_unified.py:844-858)."""
        sorted_vals, indices = probs.sort(dim=-1, descending=False)
        keep_idxs = (sorted_vals.cumsum(dim=-1) >= (1 - nucleus_prob)).nonzero(as_tuple=True)
        mask = torch.zeros_like(probs)
        mask[keep_idxs[0], indices[keep_idxs]] = 1
        return mask

    def _sampling_probs(self, logits, temperature=1.0, nucleus_prob=None):
        """Pre-sampling probability vector of `_generate_sampling` (model_unified.py:899-903): nucleus -> softmax(logits)
        times the un-renormalised nucleus mask; otherwise softmax(logits / temperature).  In the logits' dtype, like the
        reference."""
        if nucleus_prob is not None:
            probs = logits.softmax(dim=-1)
            return probs * self._get_nucleus_mask(probs, nucleus_prob)
        return (logits / temperature).softmax(dim=-1)

    @torch.no_grad()
    def _generate_sampling(self, input_embeds, attn_masks, max_len=64, num_text_per_instance=1, temperature=1.0,
                           greedy=False, nucleus_prob=None, decode_gemm=False, decode_w8=False, stop_on_eos=None, steps_out=None):
        """`_generate_sampling` (model_unified.py:861-921).  Greedy runs entirely on the device (hipGraph-replayed
        decode steps, fused argmax + log-prob), and so does sampling: `pcy_llama_sample` forms the reference's pre-sampling
        probability vector (`_sampling_probs` below is its torch restatement) and draws by inverse CDF with uniform variates
        taken from torch's device generator.
        stop_on_eos (None | eos_id): the engines' EOS stop; steps_out: a list that takes `steps_run` of every text.  Records
        of several texts per instance are padded with zeros to the longest."""
        assert nucleus_prob is None or (0 < nucleus_prob < 1)
        eng = self.text_encoder.engine
        texts = []
        for _ in range(num_text_per_instance):
            # the whole loop on the device: decode launches + the pick (greedy: argmax; sampling: softmax, nucleus mask by histogram, inverse-CDF
            # draw with uniform variates from torch's device generator); the logits record goes to the host as it is produced
            opts = dict({"decode_w8": True} if decode_w8 else {}, **({} if stop_on_eos is None else {"stop_on_eos": stop_on_eos}))
            tok, lp, lg, _ = eng.generate_greedy(input_embeds, attn_masks, max_len, keep_logits=True, decode_gemm=decode_gemm, **opts) if greedy else \
                eng.generate_sampling(input_embeds, attn_masks, max_len, temperature=temperature, nucleus_prob=nucleus_prob, keep_logits=True,
                                      decode_gemm=decode_gemm, **opts)
            texts.append((tok.cpu(), lp.cpu().clone(), lg.cpu()))
        return self._stack_texts(texts, steps_out)

    @torch.no_grad()
    def _generate_beam_search(self, input_embeds, attn_mask, max_len=64, beam_size=5, beam_group_size=5,
                              diversity_penalty=0.8, decode_gemm=False, shared_attn=False):
        """`_generate_beam_search` (model_unified.py:702-842): diverse beam search with the reference's exact
        bookkeeping (step-0 single-beam top-g, in-place Hamming penalty carried in the score, bf16 log-softmax +
        fp32 running score, EOS-anywhere stop).  The transformer steps run on the engine; the per-step
        O(B x groups) bookkeeping is `pcy_beam_step` (one launch; ties between equal candidate scores go to the lowest flat
        index, where torch.topk leaves the order unspecified)."""
        if beam_size % beam_group_size != 0:
            raise ValueError("beam_group_size must evenly divide beam_size, got: "
                             f"{beam_size} % {beam_group_size} != 0")
        if beam_size > 32:
            raise ValueError("beam_size > 32 is not supported by the device-side beam step")
        enc = self.text_encoder
        flat = enc.engine.generate_beam(input_embeds, attn_mask, max_len, beam_size, beam_group_size, diversity_penalty,
                                        self.tokenizer.eos_token_id, max_new=max(enc.max_new_tokens, max_len), decode_gemm=decode_gemm,
                                        **({"shared_attn": shared_attn} if shared_attn else {}))
        return tuple(x.unflatten(0, (input_embeds.shape[0], beam_size)) for x in flat)

    @staticmethod
    def _stack_texts(texts, steps_out=None):
        """What `_generate_sampling` and its fp32 twin return from the (tokens [B, max_len], log-prob [B], record [B, steps, V]) of every text of
        an instance, all on the host: (tokens [B, texts, max_len], log-probs [B, texts], records [B, texts, steps, V], padded with zeros to the
        longest: they differ only under an EOS stop).  steps_out takes the `steps` of every text."""
        toks, lps, recs = zip(*texts)
        if steps_out is not None:
            steps_out.extend(r.shape[1] for r in recs)
        n = max(r.shape[1] for r in recs)
        recs = [r if r.shape[1] == n else torch.nn.functional.pad(r, (0, 0, 0, n - r.shape[1])) for r in recs]
        # one text per instance (every caller in the reference): a view instead of a host-to-host copy of the [B, max_len, V] record
        # (4.2 GB at batch 32 x 512 tokens)
        return torch.stack(toks, 1), torch.stack(lps).T, recs[0].unsqueeze(1) if len(recs) == 1 else torch.stack(recs, 1)

    @contextmanager
    def _room_for(self, max_len):
        """the text encoder's caches hold at least max_len generated tokens inside the block (max_new_tokens raised, then put back)"""
        enc, keep_new = self.text_encoder, self.text_encoder.max_new_tokens
        enc.max_new_tokens = max(keep_new, max_len)
        try:
            yield
        finally:
            enc.max_new_tokens = keep_new

    # ---- fp32 generation (/root/reference/scripts/caption_bulk.py:70-73 never casts the model and calls generate(method="beam")): the
    # reference's own loops over the sub-module waist, every operator on the fp32 family (procyon_amd/engine_f32.py) -- by default a
    # compatibility path, one launch per operator and a host round trip per step, not a fast one; decode_f32="stream" puts the cached steps
    # on the device-resident step of DESIGN.md 4.10 (greedy: the whole loop on the device)
    @torch.no_grad()
    def _generate_sampling_f32(self, input_embeds, attn_masks, max_len=64, num_text_per_instance=1, temperature=1.0, greedy=False,
                               nucleus_prob=None, decode_f32="ops", stop_on_eos=None, steps_out=None):
        """`_generate_sampling` (model_unified.py:861-921) in fp32: prefill, then max_len - 1 cached steps; greedy argmax, or multinomial
        on softmax(logits / temperature) / the un-renormalised nucleus-masked softmax; chosen log-probabilities summed; no EOS stop.
        decode_f32="stream": the cached steps on the device-resident step -- greedy entirely on the device
        (`LlamaEngineF32.greedy_steps`), sampling with this loop's host-side selection around the replayed graph.
        decode_f32="device": greedy as "stream"; sampling entirely on the device too (`LlamaEngineF32.generate_sampling`).
        stop_on_eos (None | eos_id): the device-resident loops take the engines' EOS stop; the host-driven loop ("ops", and
        the sampling of "stream") checks the tokens it reads anyway -- a finished row emits eos_id and keeps its sum, the loop ends with the
        step in which the last row finishes.  steps_out: a list that takes `steps_run` of every text."""
        assert nucleus_prob is None or (0 < nucleus_prob < 1)
        enc = self.text_encoder
        B = len(input_embeds)
        stream = decode_f32 in ("stream", "device")
        prefill = lambda: enc(input_embeds=input_embeds, attn_masks=attn_masks, use_cache=True,
                              logit_positions=torch.full((B,), input_embeds.shape[1] - 1))

        def device_sampling():
            tok, lp, lg, _ = enc.engine_f32.generate_sampling(input_embeds, attn_masks, max_len, temperature=temperature, nucleus_prob=nucleus_prob,
                                                              keep_logits=True, **({} if stop_on_eos is None else {"stop_on_eos": stop_on_eos}))
            return tok.cpu(), lp.cpu(), lg.cpu()

        def device_greedy():      # the prefill through the text encoder: it sizes the cache by max_new_tokens
            eng = enc.engine_f32
            o = prefill()
            past = o.past_key_values
            st = eng.new_gen_state(B, max_len, keep_logits=True, **({} if stop_on_eos is None else {"eos_id": stop_on_eos}))
            st.logits.copy_(o.logits[:, -1, :])
            st.set(pos=past.t, step=0)
            if max_len > 1 and past.t + max_len - 1 > past.cache.Tmax:
                raise ValueError(f"KV cache capacity {past.cache.Tmax} exhausted; raise max_new_tokens")
            # the prefill's logits: token 0, the position stays; then the steps (LlamaEngineF32.greedy_from_logits)
            tok, lp, lg = eng.greedy_from_logits(past.cache, st, B, max_len, graph=True)
            return tok.cpu(), lp.cpu(), lg.cpu()

        def host_loop():
            toks, past, rec = None, None, []
            total = torch.zeros(B, device=self.device)
            fin = None if stop_on_eos is None else torch.zeros(B, dtype=torch.bool, device=self.device)
            for i in range(max_len):
                o = prefill() if i == 0 else enc(input_ids=toks[:, -1:], use_cache=True, past_key_values=past)
                past = o.past_key_values
                if stream and past.state is None:
                    past.state = enc.engine_f32.new_gen_state(B, max_len)
                logits = o.logits[:, -1, :]
                rec.append(logits.cpu())
                lsm = logits.log_softmax(-1)
                nxt = logits.argmax(-1, keepdim=True) if greedy else torch.multinomial(self._sampling_probs(logits, temperature, nucleus_prob), 1)
                if stop_on_eos is None:
                    total += lsm.gather(1, nxt)[:, 0]
                else:      # a finished row emits the EOS and keeps its sum; the row that emits it now still adds its log-probability
                    nxt = torch.where(fin[:, None], torch.full_like(nxt, stop_on_eos), nxt)
                    total = torch.where(fin, total, total + lsm.gather(1, nxt)[:, 0])
                    fin = fin | (nxt[:, 0] == stop_on_eos)
                toks = nxt if toks is None else torch.cat([toks, nxt], -1)
                if stop_on_eos is not None and bool(fin.all()):      # (the loop reads the tokens on the host anyway)
                    toks = torch.nn.functional.pad(toks, (0, max_len - toks.shape[1]), value=stop_on_eos)
                    break
            return toks.cpu(), total.cpu(), torch.stack(rec, 1)

        one_text = device_sampling if decode_f32 == "device" and not greedy else device_greedy if stream and greedy else host_loop
        with self._room_for(max_len):
            return self._stack_texts([one_text() for _ in range(num_text_per_instance)], steps_out)

    @torch.no_grad()
    def _generate_beam_search_f32(self, input_embeds, attn_mask, max_len=64, beam_size=5, beam_group_size=5, diversity_penalty=0.8, decode_f32="ops"):
        """`_generate_beam_search` (model_unified.py:702-842) in fp32: the prompt repeated beam_size times before the prefill; step 0 extends
        beam 0 of every group only, later steps the group's g x V candidates; groups after the first lose penalty x (count of the tokens
        the earlier groups of the same input chose this step) IN the running score; outputs, scores, the logits record and the K / V rows
        follow the selected parents; stops when every beam holds an EOS."""
        if beam_size % beam_group_size != 0:
            raise ValueError(f"beam_group_size must evenly divide beam_size, got: {beam_size} % {beam_group_size} != 0")
        enc = self.text_encoder
        if decode_f32 == "device":      # the whole search on the device: one prefill per prompt, no host-side selection
            flat = enc.engine_f32.generate_beam(input_embeds, attn_mask, max_len, beam_size, beam_group_size, diversity_penalty,
                                                self.tokenizer.eos_token_id, max_new=max(enc.max_new_tokens, max_len))
            return tuple(x.unflatten(0, (input_embeds.shape[0], beam_size)) for x in flat)
        dev = self.device
        B = input_embeds.shape[0]
        BB, V, T = B * beam_size, enc.cfg.vocab, input_embeds.shape[1]
        groups = beam_size // beam_group_size
        emb = torch.repeat_interleave(input_embeds, beam_size, dim=0)
        mask = torch.repeat_interleave(attn_mask, beam_size, dim=0)
        cur = torch.zeros(BB, device=dev)
        out = torch.zeros(BB, max_len, dtype=torch.int64, device=dev)
        rec = None
        with self._room_for(max_len):
            past = None
            for i in range(max_len):
                o = enc(input_embeds=emb, attn_masks=mask, use_cache=True, logit_positions=torch.full((BB,), T - 1)) if i == 0 else \
                    enc(input_ids=out[:, i - 1:i], use_cache=True, past_key_values=past)
                past = o.past_key_values
                if decode_f32 == "stream" and past.state is None:      # every cached step: the replayed graph of the stream step
                    past.state = enc.engine_f32.new_gen_state(BB, max_len)
                logits = o.logits[:, -1, :]
                step_rec = logits.cpu().unsqueeze(1)
                rec = step_rec if rec is None else torch.cat([rec, step_rec], 1)
                lp = logits.log_softmax(-1) + cur[:, None]
                src = torch.arange(BB, device=dev)
                for b in range(B):
                    b0 = b * beam_size
                    for gi in range(groups):
                        g0 = b0 + gi * beam_group_size
                        g1 = g0 + beam_group_size
                        cand = lp[g0:(g0 + 1 if i == 0 else g1)]
                        if gi != 0:
                            cand -= diversity_penalty * torch.bincount(out[b0:g0, i], minlength=V).to(dev)
                        top_v, top_i = cand.ravel().topk(beam_group_size)
                        parents = top_i // V + g0
                        out[g0:g1] = out[parents]
                        out[torch.arange(g0, g1), i] = top_i % V
                        cur[g0:g1] = top_v
                        rec[g0:g1] = rec[parents.cpu()]
                        src[g0:g1] = src[parents]        # (the K / V rows of every layer follow the parents, :830-832)
                past.cache.reorder_(src, past.t)
                if bool((out == self.tokenizer.eos_token_id).any(dim=1).all()):
                    break
        return (out.cpu().unflatten(0, (B, beam_size)), cur.cpu().unflatten(0, (B, beam_size)), rec.unflatten(0, (B, beam_size)))

    @torch.no_grad()
    def generate(self, inputs, max_len=64, aaseq_type='protein', method="sampling", temperature=1.0, greedy=False,
                 num_text_per_instance=1, return_all_internals=False, beam_size=5, beam_group_size=5,
                 diversity_penalty=0.8, exclude_protein_structure=False, nucleus_prob=0.9, truncate_on_eos=True,
                 lookahead=0, lookahead_ngram=(3, 1), decode_gemm=False, shared_attn=False, decode_w8=False, lookahead_step="extend",
                 decode_f32="ops", stop_on_eos=False):
        """`generate` (model_unified.py:924-1027).  The non-beam call site of the reference mis-binds its positional
        arguments (:998-1005, quirk Q8); the evident intent -- the same names bound by keyword -- is implemented, which
        means `nucleus_prob` (default 0.9) reaches `_generate_sampling` for every non-beam method, as written there;
        pass nucleus_prob=None for plain temperature sampling.
        lookahead=W >= 2 (not in the reference; 0, the default, is today's code): greedy generation of ONE prompt that checks W - 1 drafted
        tokens per pass over the weights (`LlamaEngine.generate_lookahead`; drafts by looking the last `lookahead_ngram` = (longest, shortest)
        tokens up in the prompt and the text so far).  Same return values; with return_all_internals the dictionary gains "lookahead" =
        {passes, tokens, accepted, tokens_per_pass}.  Its tokens do not depend on the drafts, but are not promised equal to lookahead=0
        where two logits tie within the arithmetic's noise.
        lookahead_step="extend" | "window" (with lookahead only; "extend", the default, is today's code): what a pass runs on -- the cache
        extension, or the batched decode loop with the window attention (`LlamaEngine.decode_window`).  The internals'
        "lookahead" dictionary names a step other than the default under "step".  ValueError for any other value, or for "window" without lookahead;
        NotImplementedError on the fp32 family.
        decode_gemm=True | "auto" (not in the reference; False, the default, is today's code): the cached decode steps of every method on the
        step that reads the weights once whatever the row count (`LlamaEngine.decode_gemm`) -- for more than 32 rows per step
        (prompts x beams); "auto" takes it from `engine.decode_gemm_plan`'s row count on.  Same return values; the tokens are not promised equal
        to decode_gemm=False where two logits tie within the arithmetic's noise.  Not together with lookahead (ValueError: one prompt, one
        row); not on the fp32 family (NotImplementedError).
        shared_attn=True (not in the reference; False, the default, is today's code): beam search only, together with decode_gemm -- the
        attention of the GEMM step scores all beams of a prompt against one pass over the K / V they share.  ValueError with
        any other method, with lookahead, or (from the engine, before any decode step) where the call does not run the GEMM step on the
        shared-prefix cache; NotImplementedError on the fp32 family.  Never a silent fallback.
        shared_attn="split" (not in the reference): beam search only, with or without decode_gemm -- every decode step's attention is the
        split-key one: the beams of a prompt share one pass over its K / V, softmax statistics per key chunk, two launches per
        layer.  Another rounding order than shared_attn=False (no worse against float64), so tokens may differ where two logits tie within the
        noise.  ValueError with any other method, with lookahead or decode_w8, or (from the engine, before any decode step) where the beams do
        not run on the shared-prefix cache; NotImplementedError on the fp32 family.  Any value but False, True or "split" is a ValueError.
        decode_w8=True (not in the reference; False, the default, is today's code): greedy and sampling methods only, up to 8 prompts -- the
        cached decode steps stream the e4m3 copies of the projection weights (`LlamaEngine.decode_w8`, DESIGN.md 4.3e: weight-only fp8, half
        the weight bytes per step; the prefill stays what the engine's `set_fp8` says).  The tokens are those of a model whose projection
        weights are rounded to e4m3 per output channel, not those of decode_w8=False.  ValueError together with lookahead, decode_gemm or
        method="beam", with more than 8 rows, or with anything but False / True; NotImplementedError on the fp32 family.
        decode_f32="ops" | "stream" (fp32 models only; "ops", the default, is today's code): what the cached steps of an fp32 generation run
        on.  "stream": the device-resident step on the streaming fp32 GEMV (`LlamaEngineF32.decode_stream`) -- greedy runs
        entirely on the device, sampling / nucleus and beam keep their host-side selection around one replayed graph per step.  Same return
        values; the sums run in another order than "ops", so tokens may part where two logits tie within fp32 noise.
        "device": the same step, and the selection on the device as well -- beam search is
        `LlamaEngineF32.generate_beam` (one prefill per prompt, pcy_f32_beam_step, the K / V reorder of the generated suffix, one replayed
        chain per step), sampling / temperature / nucleus `LlamaEngineF32.generate_sampling` (pcy_f32_sample_pick; the draw is the inverse
        CDF on uniform variates from torch's device generator, not torch.multinomial's stream), greedy exactly the "stream" path.  Same
        return values and shapes; beam_size <= 32.  ValueError for any other value, for "stream" / "device" on a bf16 model and for
        beam_size > 32 with "device": never a fallback.
        stop_on_eos=True (not in the reference; False, the default, is today's code: every method runs max_len steps and truncate_on_eos cuts
        the text on the host): the greedy and sampling methods end where the text ends -- the picks mark a row that emits
        the tokenizer's EOS as finished and raise a flag on the device once every row has, the host enqueues the steps in chunks of 8 and
        stops at the flag (at most 15 decode steps behind the finishing one; lookahead: none; the host-driven fp32 loops: none).  On every
        decode path: bf16 and fp32 ("ops", "stream", "device"), lookahead, decode_gemm, decode_w8.  A row's tokens up to its EOS and its
        log-probability are those of stop_on_eos=False bit for bit, every slot behind an EOS holds the EOS, the logits record is cut to
        [B, texts, steps_run, V], `text` under truncate_on_eos is the same, and return_all_internals gains "steps_run" (a list, one entry
        per text of an instance).  ValueError with method="beam" (beam search has its own stop) and for anything but False / True."""
        if not (stop_on_eos is False or stop_on_eos is True):
            raise ValueError(f"generate: stop_on_eos={stop_on_eos!r}: False or True")
        if stop_on_eos and method == "beam":
            raise ValueError("generate: stop_on_eos ends greedy and sampling generation; method='beam' has its own EOS stop")
        if not (isinstance(decode_f32, str) and decode_f32 in ("ops", "stream", "device")):
            raise ValueError(f"generate: decode_f32={decode_f32!r}: 'ops', 'stream' or 'device'")
        if decode_f32 != "ops" and not self._f32:
            raise ValueError(f"generate(decode_f32={decode_f32!r}) is the decode step of the fp32 family: this model runs the bf16 engine")
        if decode_f32 == "device" and method == "beam" and beam_size > 32:
            raise ValueError("generate(decode_f32='device'): beam_size > 32 is not supported by the device-side beam step")
        assert method in ["sampling", "temperature", "greedy", "beam", "nucleus"]
        self._require_bf16_or_fp32("generate")      # fp32 (a caller that never called .bfloat16()): the operator-by-operator fp32 loops below
        lookahead = int(lookahead)
        if lookahead and self._f32:
            raise NotImplementedError("generate(lookahead=W) needs the bf16 engine (the fp32 family has no cache extension)")
        if lookahead and (lookahead < 2 or lookahead > 32):
            raise ValueError(f"generate: lookahead={lookahead}: 0 (off) or a window of 2..32 rows")
        if lookahead_step not in ("extend", "window"):
            raise ValueError(f"generate: lookahead_step={lookahead_step!r}: 'extend' or 'window'")
        if lookahead_step != "extend" and self._f32:
            raise NotImplementedError("generate(lookahead_step=...) needs the bf16 engine (the fp32 family has no lookahead)")
        if lookahead_step != "extend" and not lookahead:
            raise ValueError(f"generate: lookahead_step={lookahead_step!r} chooses the pass of lookahead=W: pass a window too")
        if decode_gemm not in (False, True, "auto"):
            raise ValueError(f"generate: decode_gemm={decode_gemm!r}: False, True or 'auto'")
        if decode_gemm and lookahead:
            raise ValueError("generate: decode_gemm serves steps of many rows, lookahead one prompt: pass one of them")
        if decode_gemm and self._f32:
            raise NotImplementedError("generate(decode_gemm=...) needs the bf16 engine (the fp32 family has no GEMM decode step)")
        if not (shared_attn is False or shared_attn is True or (isinstance(shared_attn, str) and shared_attn == "split")):
            raise ValueError(f"generate: shared_attn={shared_attn!r}: False, True or 'split'")
        if shared_attn == "split" and decode_w8 is not False:
            raise ValueError("generate: shared_attn='split' serves beam search, decode_w8 the greedy and sampling steps: pass one of them")
        if shared_attn and self._f32:
            raise NotImplementedError("generate(shared_attn=True) needs the bf16 engine (the fp32 family has no shared-prefix cache)")
        if shared_attn and lookahead:
            raise ValueError("generate: shared_attn serves the beams of a beam search, lookahead one greedy row: pass one of them")
        if shared_attn and method != "beam":
            raise ValueError(f"generate: shared_attn scores the beams of a prompt together: method='beam' only, got {method!r}")
        if decode_w8 is not False:
            if decode_w8 is not True:
                raise ValueError(f"generate: decode_w8={decode_w8!r}: False or True")
            if self._f32:
                raise NotImplementedError("generate(decode_w8=True) needs the bf16 engine (the fp32 family has no e4m3 decode step)")
            if lookahead or decode_gemm or method == "beam":
                raise ValueError("generate: decode_w8 serves the greedy and sampling steps of up to 8 rows: not together with lookahead, decode_gemm or method='beam'")
            n_rows = len(inputs.get("instructions") or ()) if isinstance(inputs, dict) else 0
            if n_rows > 8:
                raise ValueError(f"generate: decode_w8 serves 1..8 rows, got {n_rows} prompts")
        if method == "beam":
            num_text_per_instance = beam_size
        elif method == "greedy":
            greedy = True
        elif method in ["sampling", "nucleus"]:
            temperature = 1
        if temperature < 1e-8:
            greedy = True
        input_embeds, input_ids, attn_masks, _, _, _ = self._preprocessing(
            inputs, aaseq_type=aaseq_type, crop_off=True, no_pad=True,
            exclude_protein_structure=exclude_protein_structure, left_pad=True)
        whole_instructions = self.tokenizer.batch_decode(input_ids)
        gt_text = [inputs["data"]["text"][i] for i in inputs["target"]["text"]] if inputs["target"]["text"] is not None else None
        batch_size = input_embeds.shape[0]
        look_stats = None
        steps_run = []
        stop = {"stop_on_eos": int(self.tokenizer.eos_token_id)} if stop_on_eos else {}
        if lookahead:
            if method == "beam" or not greedy:
                raise ValueError("generate(lookahead=W) verifies drafts against the argmax: it needs a greedy method (method='greedy' or greedy=True)")
            if batch_size != 1 or num_text_per_instance != 1:
                raise ValueError(f"generate(lookahead=W): one prompt and one text at a time, got {batch_size} prompts x {num_text_per_instance} texts")
            # soft-token slots hold no text: negative in the history, so they never match and are never drafted
            hist_ids = input_ids[0].clone()
            for i in (self.prot_replacement_idx, self.struct_idx, self.drug_idx):
                hist_ids[hist_ids == i] = -1
            tok, lp, lg, (_, _, look) = self.text_encoder.engine.generate_lookahead(input_embeds, hist_ids, max_len, lookahead, ngram=lookahead_ngram,
                                                                                    keep_logits=True, **({} if lookahead_step == "extend" else {"step": lookahead_step}),
                                                                                    **stop)
            steps_run.append(lg.shape[1])
            tokens, log_probs, logits = tok.cpu().unsqueeze(1), lp.cpu().clone().unsqueeze(0).T, lg.cpu().unsqueeze(1)
            # ("step" is named only where it was chosen: the default call returns the dictionary it always returned)
            look_stats = look.stats() if lookahead_step == "extend" else dict(look.stats(), step=lookahead_step)
        elif method == "beam":
            tokens, log_probs, logits = (self._generate_beam_search_f32 if self._f32 else self._generate_beam_search)(
                input_embeds, attn_masks, max_len=max_len, beam_size=beam_size, diversity_penalty=diversity_penalty,
                beam_group_size=beam_group_size, **({"decode_gemm": decode_gemm} if decode_gemm else {}),
                **({"shared_attn": shared_attn} if shared_attn else {}), **({"decode_f32": decode_f32} if decode_f32 != "ops" else {}))
        else:
            tokens, log_probs, logits = (self._generate_sampling_f32 if self._f32 else self._generate_sampling)(
                input_embeds, attn_masks, max_len=max_len, num_text_per_instance=num_text_per_instance,
                temperature=temperature, greedy=greedy, nucleus_prob=nucleus_prob, **({"decode_gemm": decode_gemm} if decode_gemm else {}),
                **({"decode_w8": True} if decode_w8 else {}), **({"decode_f32": decode_f32} if decode_f32 != "ops" else {}),
                **(dict(stop, steps_out=steps_run) if stop else {}))
        flattened = torch.flatten(tokens, start_dim=0, end_dim=1)
        text = self.tokenizer.batch_decode(flattened)
        if truncate_on_eos:
            text = [x.split(self.tokenizer.eos_token)[0].strip() for x in text]
        text = [text[i * num_text_per_instance:(i + 1) * num_text_per_instance] for i in range(batch_size)]
        if return_all_internals:
            out = {"out_tokens": tokens, "out_logits": logits, "out_log_probs": log_probs, "text": text,
                   "input_instructions": whole_instructions, "ground_truth_text": gt_text,
                   "text_references": inputs["reference_indices"]["target"]["text"],
                   "seq_references": [inputs["reference_indices"]["input"]["seq"][j][-1] for j, _ in enumerate(inputs["input"]["seq"])]}
            if look_stats is not None:
                out["lookahead"] = look_stats
            if stop_on_eos:
                out["steps_run"] = steps_run
            return out
        return tokens, log_probs, logits, text
