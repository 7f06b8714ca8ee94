"""Child of tests/test_gpu_attention_stream.py: the causal forward and backward
of attention_stream_cases.ORDER_CASES in the block order this process was
started with (TDFO_ATTN_CAUSAL_ORDER=natural), written to argv[1] as a list of
{out, lse, dqkv}."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from tdfo_amd.ops import _ext  # noqa: E402
from tests import attention_stream_cases as sc  # noqa: E402

assert os.environ.get(sc.ORDER_ENV) == "natural", "start with the natural block order"
assert torch.cuda.is_available() and _ext.load()
res = []
for case in sc.ORDER_CASES:
    c = sc.stream_case(*case)
    assert c.causal
    res.append(sc.run_stream(c))
torch.save(res, sys.argv[1])
print(f"{len(res)} cases in the natural order", flush=True)
