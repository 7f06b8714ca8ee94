"""What ops says about the fused top-K search's widths without a GPU."""
import torch

from tdfo_amd import ops
from tests.retrieval_cases import brute_force, exact_case


def test_topk_fused_widths():
    assert tuple(ops.topk_fused_widths()) == (16, 32, 64, 128, 256)
    assert not hasattr(ops, "TOPK_FALLBACK_E")


def test_cpu_tensors_keep_the_reference_at_wide_e():
    """CPU tensors at E = 128 go through ops.topk_scores to the chunked
    reference: equal to a brute-force sort in fp64 (the case is exact)."""
    c = exact_case(128, 5, 300, 10, 20)
    ids, scores, rank = brute_force(c["q"], c["W"], c["bias"], 10, c["v_lo"], c["v_hi"],
                                    c["exclude"], c["target"])
    assert torch.equal(c["ids"], ids) and torch.equal(c["scores"], scores)
    assert torch.equal(c["rank"], rank)
