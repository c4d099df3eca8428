"""CPU: the float64 restatement of the RNN language model (tests/rnn_lm_f64.py) against the
reference's own outputs, and the fp32 figures behind the GPU bounds.

tests/golden/rnn_lm_ref.npz was written by the reference's RnnLm and MaskedKLDivergence running in
float32 (tools/gen_golden.py rnn_lm), so the restatement in float64 on the fixture's float32
parameters differs from it by the fixture's own float32 rounding: a few operations deep at
V = 16, E = H = 8, T = 9, i.e. a few times 2^-24 = 6e-8 relative to a tensor's largest entry.
Measured (max |restatement - fixture| / max |fixture|): logits 1.1e-7, score 4.5e-8, score_step
log-probs / states <= 1.2e-7, loss 6.5e-8, gradients <= 2.2e-7.  TOL = 2e-6 is 32 x 2^-24: ten times the
largest figure, and a thousand times below what a wrong gate order or a dropped bias gives.
"""
import json
import os

import numpy as np
import pytest
import torch

import rnn_lm_cases as LC
import rnn_lm_f64 as RF

TOL = 2e-6
LABEL_SMOOTHING = 0.1


@pytest.fixture(scope="module")
def fix(golden_dir):
    z = np.load(os.path.join(golden_dir, "rnn_lm_ref.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]).double() for k in z.files if k.startswith("sd.")}
    return z, sd, torch.from_numpy(z["tokens"]), torch.from_numpy(z["lengths"])


def _hold(what, got, ref):
    err = LC.rel_err(got, torch.as_tensor(np.asarray(ref)))
    print(f"{what}: err {err:.3e}")
    assert err <= TOL, (what, err)


def test_fixture_is_the_tiny_config_of_the_issue(fix):
    z, sd, tokens, lens = fix
    assert tokens.shape == (4, 9) and lens.tolist() == [9, 7, 5, 2]
    assert sd["_embedding.weight"].shape == (16, 8) and RF.num_layers(sd) == 2
    assert sd["_rnn_layer.weight_hh_l1"].shape == (32, 8)
    assert sd["_logits_layer.weight"].shape == (16, 8)
    assert all(z[k].dtype == np.float32 for k in z.files if k.startswith(("sd.", "grad.")))


def test_forward_and_score_equal_the_reference(fix):
    z, sd, tokens, lens = fix
    logits, _ = RF.logits_ref(sd, tokens)
    _hold("logits", logits, z["logits"])
    _hold("score", RF.score_ref(sd, tokens, lens), z["score"])


def test_two_chained_score_steps_equal_the_reference(fix):
    z, sd, tokens, _ = fix
    B, L, H = tokens.shape[0], RF.num_layers(sd), sd["_embedding.weight"].shape[1]
    st = (torch.zeros(L, B, H, dtype=torch.float64), torch.zeros(L, B, H, dtype=torch.float64))
    for i in range(2):
        lp, st = RF.score_step_ref(sd, tokens[:, i], st)
        _hold(f"step{i} log_probs", lp, z[f"step{i}_log_probs"])
        _hold(f"step{i} h", st[0], z[f"step{i}_h"])
        _hold(f"step{i} c", st[1], z[f"step{i}_c"])
    # a step continues the sequence: two steps = the first two positions of forward
    logits, _ = RF.logits_ref(sd, tokens)
    assert LC.rel_err(lp, torch.log_softmax(logits[:, 1], -1)) < 1e-14


def test_training_loss_and_every_gradient_equal_the_reference(fix):
    z, sd, tokens, lens = fix
    loss, grads = RF.grads_ref(sd, lambda s: RF.nnlm_loss_ref(s, tokens, lens, LABEL_SMOOTHING))
    _hold("loss", loss, z["loss"])
    assert set(grads) == {k[5:] for k in z.files if k.startswith("grad.")}
    for k, g in grads.items():
        _hold("d " + k, g, z["grad." + k])
    assert torch.equal(grads["_rnn_layer.bias_ih_l0"], grads["_rnn_layer.bias_hh_l0"])


def test_padded_positions_do_not_reach_the_loss(fix):
    _, sd, tokens, lens = fix
    a = RF.nnlm_loss_ref(sd, tokens, lens, LABEL_SMOOTHING)
    t2 = tokens.clone()
    for b in range(t2.shape[0]):
        t2[b, lens[b]:] = 7
    assert torch.equal(a, RF.nnlm_loss_ref(sd, t2, lens, LABEL_SMOOTHING))


def test_top_k_accuracy_counts_the_valid_positions_only():
    logits = torch.zeros(2, 3, 5, dtype=torch.float64)
    logits[0, 0, 2] = 1.0       # hit at k = 1
    logits[0, 1, 3] = 1.0
    logits[0, 1, 4] = 0.5       # label 4: a hit at k = 2 only
    logits[1, 0, 1] = 1.0       # label 4: a miss at k = 1 and at k = 2 (the runner-up is class 0)
    logits[1, 0, 0] = 0.5
    logits[1, 1, 0] = 1.0       # beyond the length: not counted
    labels = torch.tensor([[2, 4, 0], [4, 0, 0]])
    lens = torch.tensor([2, 1])
    assert abs(float(RF.topk_acc_ref(logits, labels, lens, 1)) - 1 / 3) < 1e-6
    assert abs(float(RF.topk_acc_ref(logits, labels, lens, 2)) - 2 / 3) < 1e-6


def test_stack_keep_masks_follow_every_layer_but_the_last(fix):
    _, sd, tokens, _ = fix
    x = torch.nn.functional.embedding(tokens.t(), sd["_embedding.weight"])
    g = torch.Generator().manual_seed(5)
    keep = [(torch.rand(9, 4, 8, generator=g) < 0.7).double() / 0.7]
    y, _ = RF.stack_ref(x, sd, keep=keep)
    p = "_rnn_layer."
    h1, _, _ = RF.lstm_ref(torch.nn.functional.linear(x, sd[p + "weight_ih_l0"], sd[p + "bias_ih_l0"] + sd[p + "bias_hh_l0"]),
                           sd[p + "weight_hh_l0"])
    h2, _, _ = RF.lstm_ref(torch.nn.functional.linear(h1 * keep[0], sd[p + "weight_ih_l1"], sd[p + "bias_ih_l1"] + sd[p + "bias_hh_l1"]),
                           sd[p + "weight_hh_l1"])
    assert torch.equal(y, h2)


@pytest.mark.parametrize("name", ["h4_b1_t1_state", "h20_b15_t2", "h64_b16_t9", "sat100"])
def test_cell_equals_torch_lstm_in_float64(name):
    t = LC.make(name)
    a, b = LC.reference(name), LC.evaluate_nn_lstm(t, torch.float64)
    for k in LC.TENSORS_FWD + LC.TENSORS_BWD:
        assert LC.rel_err(b[k], a[k]) < 1e-13, k


def test_state_keys_fixture_is_the_yaml_config(golden_dir):
    keys = json.load(open(os.path.join(golden_dir, "state_keys_nnlm.json")))
    assert len(keys) == 15 and keys["_nnlm._embedding.weight"] == [128, 512]
    assert keys["_nnlm._rnn_layer.weight_hh_l2"] == [2048, 512]
    assert keys["_nnlm._logits_layer.bias"] == [128]


# ------------------------------------------------------------------ what fp32 costs the reference
@pytest.mark.parametrize("name", list(LC.CASES))
def test_fp32_cost_of_the_reference(name):
    """torch.nn.LSTM in float32 on the CPU against the float64 restatement, forward and backward,
    on the case's inputs.  As in test_lstm_f64.py the figure is a maximum over a tensor and moves
    with the host, so the check is of the order of magnitude, both ways: the measurement within
    4 x the record and the record within 4 x the measurement."""
    ref = LC.reference(name)
    for k, v in ref.items():
        assert torch.isfinite(v).all(), k
    fwd, bwd = LC.fp32_figures(name)
    print(f"fp32 cost {name}: fwd={fwd:.3e} bwd={bwd:.3e}")
    rec = LC.FP32_COST[name]
    assert fwd <= 4 * rec["fwd"] and bwd <= 4 * rec["bwd"], (fwd, bwd, rec)
    assert rec["fwd"] <= 4 * fwd and rec["bwd"] <= 4 * bwd, (fwd, bwd, rec)


def test_case_inputs_are_what_the_table_says():
    for name, c in LC.CASES.items():
        t = LC.make(name)
        assert t["gx"].shape == (c["T"], c["B"], 4 * c["H"]) and t["gx"].dtype == torch.float32
        if c["spike"]:
            share = (t["gx"].abs() == c["spike"]).float().mean().item()
            assert 0.005 <= share <= 0.011 and t["gx"].max() == c["spike"] and t["gx"].min() == -c["spike"]
        assert (t["h0"] is not None) == c["state"]
    assert set(LC.CASES) == set(LC.FP32_COST)
    assert set(LC.STEP_CASES + LC.AUTO_CASES + LC.SEQ_CASES + LC.COMPOSED_CASES) == set(LC.CASES)
    assert [LC.CASES[k]["B"] for k in LC.AUTO_CASES] == [LC.THRESHOLD]
