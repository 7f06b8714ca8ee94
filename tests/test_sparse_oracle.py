"""CPU self-check of tests/sparse_oracle.py: every shape of the GPU width
tests (embedding forward, fused embedding backward, interaction) runs through
``ops.*`` on CPU tensors -- the fp32 torch references -- and must meet the
same tolerances as the HIP kernels, with no element exempted. That shows the
float64 oracles agree with the project's reference and that the tolerances do
not need a kernel's help."""
import pytest
import torch

from tdfo_amd import ops
from tests import sparse_oracle as so

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}


@pytest.mark.parametrize("mode", so.FWD_MODES, ids=lambda m: f"{m[0]}-psw{int(m[1])}-mean{int(m[2])}")
@pytest.mark.parametrize("D", so.WIDTHS)
def test_fwd_multihot_reference_within_bound(D, mode):
    dt, use_psw, mean = mode
    c = so.fwd_multihot_case(D)
    out = so.run_fwd(c, "cpu", DT[dt], use_psw, mean)
    oracle = so.embedding_bag_fwd(c["W"], c["ro"], c["idx"], c["offs"], c["out_off"], c["T"],
                                  c["B"], c["out_stride"], psw=c["psw"] if use_psw else None,
                                  mean=mean)
    assert so.check_fwd(out, oracle) <= 1.0
    assert int(oracle[2].max()) == 130 and int(oracle[2][oracle[3]].min()) == 0


@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("use_psw", [False, True])
@pytest.mark.parametrize("D", so.WIDTHS)
def test_fwd_onehot_reference_within_bound(D, use_psw, large):
    c = so.fwd_onehot_case(D, large)
    out = so.run_fwd(c, "cpu", torch.bfloat16 if D <= 64 else torch.float32, use_psw, False)
    so.check_fwd(out, so.fwd_onehot_oracle(c, use_psw))
    if large:
        assert c["T"] * c["B"] > 8192 * 4 * so.fwd_onehot_bpw(D)


def _bwd_check(c, opt, hyper=None):
    st = so.bwd_states(c, opt)
    got = so.run_bwd(c, opt, "cpu", [None if s is None else s.clone() for s in st], hyper=hyper)
    return so.check_bwd(got, so.bwd_before(c, st), c["urows"], so.bwd_exact(c, opt, st, hyper),
                        c["D"])


@pytest.mark.parametrize("path", range(len(so.BWD_PATHS)), ids=[p[0] for p in so.BWD_PATHS])
@pytest.mark.parametrize("opt", so.ALL_OPTS)
@pytest.mark.parametrize("D", so.WIDTHS)
def test_bwd_reference_within_tolerance(D, opt, path):
    _bwd_check(so.bwd_case(D, path), opt)


@pytest.mark.parametrize("opt", [ops.EMB_ROWWISE_ADAGRAD, ops.EMB_ADAM, ops.EMB_DENSE_GRAD])
@pytest.mark.parametrize("D", [16, 256, 512])
def test_bwd_long_runs_reference_within_tolerance(D, opt):
    c = so.bwd_long_case(D)
    hot = torch.bincount(c["ro"][0] + c["idx"][:c["offs"][c["B"]]], minlength=3)
    assert int(hot.min()) > 256 * 16          # past COMBINE_LONG chunks of the largest CH
    _bwd_check(c, opt)


@pytest.mark.parametrize("opt", [ops.EMB_SGD, ops.EMB_ADAM])
@pytest.mark.parametrize("D", [16, 128, 512])
def test_bwd_key64_shapes_reference_within_tolerance(D, opt):
    for c in (so.bwd_onehot_case(D, 256), so.bwd_onehot_case(D, 2304), so.bwd_multirun_case(D)):
        _bwd_check(c, opt)


@pytest.mark.parametrize("opt", [ops.EMB_ROWWISE_ADAGRAD, ops.EMB_ADAM])
@pytest.mark.parametrize("D", [16, 512])
def test_bwd_fixed_len_reference_within_tolerance(D, opt):
    _bwd_check(so.bwd_fixed_len_case(D), opt)


def test_bwd_loss_scale_reference():
    c = so.bwd_case(256, 1)
    lr, step = so.HYPER
    _bwd_check(c, ops.EMB_ADAM, hyper=torch.tensor([lr, step, 0.5, 0.0]))
    _bwd_check(c, ops.EMB_ADAM, hyper=torch.tensor([lr, step, 0.5, 1.0]))


@pytest.mark.parametrize("B", so.INTER_B)
@pytest.mark.parametrize("F", so.INTER_F)
@pytest.mark.parametrize("D", so.INTER_D)
def test_interaction_reference_within_bound(D, F, B):
    c = so.inter_case(D, F, B)
    assert so.check_inter_fwd(so.run_inter_fwd(c, "cpu"), c) <= 1.0
    if F == 17 and B == 37:
        oc = c["ones_col"]
        assert so.check_inter_fwd(so.run_inter_fwd(c, "cpu", oc), c, oc) <= 1.0
    for relu_mask in (True, False):
        dd, de = so.run_inter_bwd(c, "cpu", relu_mask)
        assert so.check_inter_bwd(dd, de, c, relu_mask) <= 1.0


def test_interaction_case_has_signed_zeros():
    x = so.inter_dense(so.inter_case(16, 2, 1)).float()
    assert bool((x == 0).any()) and bool((x < 0).any())
    assert bool((torch.signbit(x) & (x == 0)).any()) and bool((~torch.signbit(x) & (x == 0)).any())
