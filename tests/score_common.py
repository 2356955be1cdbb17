"""Shared by tests/test_gpu_score.py and its PCY_DEBUG_POISON_WS child process: one deterministic scoring workload on the small synthetic
model -> CPU tensors.  Run as a script it writes them to the path given as its argument (torch.save)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

INSTR = ["w1 <|protein|> is w2 ? [ANSWER] yes w3 w4 w5",
         "w4 <|protein|> ? [ANSWER] alpha beta gamma delta epsilon zeta eta",
         "describe w8 <|protein|> and <|protein|> now please [ANSWER] q r"]
SLOTS = [[0], [1], [0, 1]]


def build_env():
    from procyon_amd import synth
    from procyon_amd import synthetic_model as SM
    model, w = SM.build("small", device="cuda", return_weights=True, max_new_tokens=32)
    return dict(model=model, w=w, prot=synth.protein_tokens([90, 41], seed=3))


def make_inputs(env, instr=INSTR, slots=SLOTS):
    prot = env["prot"]
    return {"data": {"seq": prot, "seq_idx": torch.arange(prot.shape[0]), "text": [], "drug": None},
            "input": {"seq": [list(s) for s in slots], "text": [[] for _ in instr], "drug": None},
            "target": {"seq": None, "text": None, "drug": None}, "instructions": list(instr)}


def scoring_results(env):
    """the one-pass scoring forward + the operator on a planted input -> {name: CPU tensor}"""
    from procyon_amd.engine import Context
    m = env["model"]
    out = m.forward(make_inputs(env), compute_loss=True, get_full_labels=True)
    o = out["outputs"]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(70, 256, generator=g).to(torch.bfloat16).cuda()
    W = (torch.randn(2311, 256, generator=g) / 16).to(torch.bfloat16).cuda()
    tg = torch.randint(0, 2311, (70,), generator=g).cuda()
    parts = Context.get().lm_head_xent(x, W, tg, want_parts=True)
    res = {"token_nll": o.token_nll, "loss": o.loss, "answer_logits": o.answer_logits}
    res.update({f"xent{i}": p for i, p in enumerate(parts)})
    return {k: v.detach().cpu() for k, v in res.items()}


if __name__ == "__main__":
    torch.save(scoring_results(build_env()), sys.argv[1])
