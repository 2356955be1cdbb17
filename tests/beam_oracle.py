"""The tie-aware rule that holds a beam search of the engine to the oracle's (oracle.llama_ref.beam_search): shared by the beam tests
(test_gpu_unified.py, test_gpu_decode_wide.py).  Two bf16 pipelines need not pick the same candidates where the oracle's own candidate
scores tie within the logits noise, so every prompt's beams must equal the oracle's up to the first step at which they differ, and that
step must hold such a near-tie among the oracle's top-(g+1) candidates of that prompt."""
import torch

from conftest import rel_err


def assert_beam_matches_oracle(tokens, scores, logits, t_ref, s_ref, lg_ref, trace, step0_bar=1e-2, step_bar=2e-2):
    """tokens / scores / logits: the engine's [B, beam, L], [B, beam], [B, beam, L, V]; t_ref / s_ref / lg_ref: the oracle's; trace: the
    oracle's (step, prompt, group, top-(g+1) candidate scores) records.  Checked per prompt (prompts do not interact): step-0 logits within
    `step0_bar`, the logits record within `step_bar` wherever both searches hold the same prefixes."""
    assert tokens.shape == t_ref.shape and scores.shape == s_ref.shape
    for b in range(t_ref.shape[0]):
        # step 0 is identical up to bf16 noise: same top-2 per group from beam 0 (before any re-indexing every row of a prompt holds the
        # same logits, so this comparison does not depend on the beams' order)
        assert rel_err(logits[b, 0, 0], lg_ref[b, 0, 0]) < step0_bar, b
        noise = float((logits[b, 0, 0].float() - lg_ref[b, 0, 0].float()).abs().max())
        if torch.equal(tokens[b], t_ref[b]):
            assert torch.allclose(scores[b], s_ref[b], atol=0.3), b
            # the logits record: beam j's row at step s is what the model gave for the prefix tokens[b, j, :s]
            assert rel_err(logits[b], lg_ref[b]) < step_bar, b
            continue
        # A divergence must come from a near-tie among the oracle's own candidate scores at the FIRST step that differs: some adjacent pair
        # of its top-(g+1) candidates (bf16 log-softmax + fp32 running score) lies within the logits noise (x4, plus one bf16 ulp of the
        # score, the granularity of the log-softmax) -- otherwise the engine picked a clear loser.
        first = int((tokens[b] != t_ref[b]).any(0).nonzero()[0])
        gaps = []
        for (step, pb, k, top) in trace:
            if step == first and pb == b:
                ulp = 2.0 ** -8 * float(top.abs().max())
                gaps += [(float(g_), ulp) for g_ in (top[:-1] - top[1:])]
        assert gaps and any(g_ <= 4 * noise * (first + 1) + ulp for g_, ulp in gaps), (b, first, noise, gaps)
        assert torch.equal(tokens[b, :, :first], t_ref[b, :, :first]), b
        # up to the first difference the two searches extended the same prefixes: same logits record up to bf16 noise
        assert rel_err(logits[b, :, :first + 1], lg_ref[b, :, :first + 1]) < step_bar, (b, first)
