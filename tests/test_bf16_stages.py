"""Every stage of the bf16 matrix-core path (ppo_cpp_amd/csrc/ppo_bf16.hpp) against a float64 reference fed with that stage's own device inputs, rounding
included.  The reference, the derivation of every bound and the comparison rules are in tests/bf16_ref.py; the workspaces are read through ppo_debug_buffer
("bf_theta", "bf_x0", "bf_h_pi_0", ... include/ppo_hip.h).

What survives a call and what does not:
  * every workspace of the path survives to the end of ppo_step / ppo_train_step (they are plain device buffers written once per call), EXCEPT the operand mirror:
    `theta_bf` is rewritten by the Adam step at the end of ppo_train_step (bf16_reduce_adam_kernel: `*reinterpret_cast<bf16x4*>(a.theta_bf + idx) = o4;`, adam_kernel
    likewise), so the activations a train step leaves behind were computed with the PREVIOUS mirror.  The tests read "bf_theta" before the step (ordering trap).
  * the train pass's forward buffers (bf_x0, bf_h_*, bf_head_*) are the same buffers the act pass wrote: the act pass is checked first, then the train pass on the same
    observations must leave the same bits (act model and train model are the same launches), and the backward stages are checked against those.
  * after ppo_collect_synthetic `bf_x0` holds the BOOTSTRAP value pass's rows (enqueue_finish restages the buffer: `launch_step(h, a)` with a.obs = h->raw_obs), not
    the last rollout step's: test_rollout_staging compares against that pass's observations, and checks a rollout step's staging through ppo_rollout_act.

Observed on an MI355X (the figures every GPU test prints; largest over all cases of this module): OBSERVED below.
"""
import numpy as np
import pytest

from oracle import oracle as o
from tests import bf16_ref as R
from tests import helpers as H

gpu = pytest.mark.gpu

CR = 0.16102319955825806
LR = 0.000393141177482903
GAMMA, LAM = 0.99, 0.95
BF16 = 1
R_VF = 0.05

# (hidden, O, A, n): the smallest shapes that reach each code path (tests/test_bf16_path.py launches all of them)
CASES = {
    "tiles128_ragged_elementwise_staging": ((256, 128), 18, 18, 130),
    "work_balanced_dw_split": ((384,), 40, 7, 640),
    "head_ranges_longer_than_one_image": ((128, 2048), 18, 18, 256),
    "head_one_and_a_quarter_image_A70": ((1280,), 18, 70, 128),
    "Kp0_384_ragged_1000": ((1024, 512), 300, 100, 1000),
    "tiles256_stage4_chain": ((512, 512), 64, 18, 2048),
}

# Largest figures observed on an MI355X over all GPU tests of this module (printed by every test: `report`).  Units: the share of the derived bound E an element
# needed (bf16 outputs: to explain a rounding that is not rne(y); fp32 outputs: |out - ref| / E); 1.0 is the edge of the bound.
OBSERVED = """
    stage             units of E   share q != rne(y) (largest cap)   relative L2 (largest cap)
    hidden forward    0.123        2.14e-3   (2.14e-2)                                            the tanh form's absolute error: tests/bf16_ref.py, emu_tanh_f32
    dhead (loss)      0.0497       8.7e-4    (7.8e-2 = 10 / 128 rows)
    backward dy       0.0029       9.7e-5    (1.2e-3)
    head sums         0.0029                                         1.5e-7  (1.7e-6)
    bias sums         0.0009                                         5.7e-7  (1.7e-5)
    dW                0.0057                                         1.4e-7  (1.9e-6)
    fp32 scalars and vectors, units of E: action 0.46, neglogp 0.078, pg_loss 0.0024, vf_loss 0.0075, entropy 0.0064, approxkl 0.0036, clipfrac 0.0033, grad pi/b 0.012,
    grad pi/logstd 0.0057, grad vf/b 0.001, hidden bias gradients 0.0009, global norm 0.021, Adam m 0.025, Adam v 0.012, theta 0.999 (its bound is the weight's own final
    rounding, U |theta|, plus 8 U of the step: some element of 1e5 always sits at half an ulp).
    The worst-case accumulation bound (2 units per addition, every addition at its worst) is 10 to 300 times what the matrix unit shows: it is the exact-rounding share
    and the relative L2 error, both held to 10 x an fp32 emulation of the same stage, that would catch a subtly wrong kernel; the bracket catches a grossly wrong element.
"""


def seeded_oracle(hidden, O, A, seed=3):
    """orthogonal weights as the existing bf16 tests use, plus NON-ZERO biases (a kernel that dropped or misplaced a bias must show)"""
    orc = o.Oracle(O, A, list(hidden))
    orc.init_orthogonal(seed)
    rng = np.random.RandomState(seed + 1)
    orc.tensor("pi/logstd")[:] = rng.uniform(-1.0, 0.2, (1, A))
    for name, _, shape in orc.tensors:
        if name.endswith("/b"):
            orc.tensor(name)[:] = rng.uniform(-0.1, 0.1, shape)
    return orc


# =====================================================================================================================================================
# not GPU: the reference itself
# =====================================================================================================================================================
def test_rne_bf16_is_torch_bfloat16_bit_for_bit():
    import torch
    rng = np.random.RandomState(0)
    x = np.concatenate([rng.normal(size=300000), rng.uniform(-1e-3, 1e-3, 300000), rng.normal(size=200000) * 1e30, rng.normal(size=200000) * 1e-38]).astype(np.float32)
    edge = np.array([0x00000000, 0x80000000, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F800000, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0x7F800000, 0xFF800000,
                     0x00000001, 0x00007FFF, 0x00008000, 0x00018000, 0x007FFFFF, 0x00800000, 0x807F8000, 0xBF808000, 0xBF818000], np.uint32).view(np.float32)
    x = np.concatenate([x, edge, -edge])
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    got = R.rne_bf16(x)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[x.size - 2 * edge.size + 2] == np.float32(1.0) and got[x.size - 2 * edge.size + 3] == np.float32(1.015625)      # ties go to the even mantissa
    assert np.isinf(R.rne_bf16(np.float32([3.4e38]))[0])                                                                     # the largest finite fp32 rounds up to inf
    np.testing.assert_array_equal(R.from_bits(R.bf16_bits(got[np.isfinite(got)])), got[np.isfinite(got)])
    assert np.isnan(R.rne_bf16(np.float32([np.nan]))[0])


@pytest.mark.parametrize("mode", ["policy", "range", "off"])
@pytest.mark.parametrize("hidden,O,A,n", [((24, 16), 11, 5, 96), ((40,), 7, 3, 64)])
def test_reference_without_rounding_is_the_fp32_oracle(hidden, O, A, n, mode):
    """the stage functions of tests/bf16_ref.py chained end to end with the identity in place of rne_bf16 reproduce orc.step and orc.loss_grad (under the
    three value-clip modes: the spliced reference tests/test_value_clip.py states) at 1e-5: the reference states the right mathematics"""
    from tests import test_value_clip as VC
    orc = seeded_oracle(hidden, O, A)
    p = R.oracle_params(orc)
    rng = np.random.RandomState(7)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32); noise = rng.normal(size=(n, A)).astype(np.float32)
    f = R.chain_forward(p, obs, R.identity, A)
    ra, rv, rnlp = orc.step(obs, noise)
    act, _ = R.act_epilogue(f["mu"], p["logstd"], noise)
    np.testing.assert_allclose(act, ra, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(f["v"], rv, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(R.nlp_terms(f["mu"], p["logstd"], ra)[3], rnlp, rtol=1e-5, atol=1e-5)
    args = VC.gaussian_batch(orc, n, seed=5)
    mb = dict(zip(("obs", "actions", "advs", "returns", "old_neglogp", "old_values"), args))
    vmode = {"policy": VC.POLICY, "range": VC.RANGE, "off": VC.OFF}[mode]
    ref_losses, ref_grad = VC.spliced_loss_grad(orc, args, CR, vmode, R_VF)
    vcr, voff = {"policy": (CR, 0.0), "range": (R_VF, 0.0), "off": (0.0, np.inf)}[mode]
    losses, grads, _ = R.chain_train(p, mb, R.identity, A, float(np.float32(CR)), float(np.float32(vcr)), voff, orc.cfg.ent_coef, orc.cfg.vf_coef)
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-5, atol=1e-5)
    grad = R.flat_grad(orc.tensors, grads)
    np.testing.assert_allclose(grad, ref_grad, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(ref_grad).max()))
    assert np.abs(grad).max() > 1e-3


@pytest.mark.parametrize("seed", [3, 11, 40])
def test_synth_minibatch_is_unchanged_bit_for_bit(seed):
    """helpers.synth_minibatch now goes through helpers.synth_minibatch_from: the minibatches every existing test draws must be the same bits as before
    (the body below is the function as it was)"""
    def before(orc, n, seed, cr=CR):
        rng = np.random.RandomState(seed)
        obs = rng.uniform(-1, 1, (n, orc.O)).astype(np.float32)
        noise = rng.normal(size=(n, orc.A)).astype(np.float32)
        act, v, nlp = orc.step(obs, noise)
        old_nlp = (nlp + rng.normal(scale=0.15, size=n)).astype(np.float32)
        old_v = (v + rng.normal(scale=0.2, size=n)).astype(np.float32)
        ret = (v + rng.normal(scale=0.5, size=n)).astype(np.float32)
        ratio = np.exp(old_nlp.astype(np.float64) - nlp)
        near = np.abs(np.abs(ratio - 1.0) - cr) < 1e-3
        old_nlp[near] += np.float32(0.01)
        dvo = v.astype(np.float64) - old_v
        near = np.abs(np.abs(dvo) - cr) < 1e-3
        old_v[near] -= np.float32(0.01) * np.sign(dvo[near]).astype(np.float32)
        dvo = v.astype(np.float64) - old_v
        vclip = old_v + np.clip(dvo, -cr, cr)
        s1, s2 = (v - ret.astype(np.float64)) ** 2, (vclip - ret) ** 2
        near = (np.abs(dvo) > cr) & (np.abs(s1 - s2) < 1e-3 * np.maximum(s1, 1e-6))
        ret[near] += np.float32(0.05)
        return dict(obs=obs, actions=act, advs=o.adv_normalize(ret, old_v), returns=ret, old_neglogp=old_nlp, old_values=old_v)
    orc = seeded_oracle((32, 24), 18, 6, seed=seed)
    for n in (700, 64):
        a, b = H.synth_minibatch(orc, n, seed), before(orc, n, seed)
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].dtype == b[k].dtype
            np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=k)
    mb = H.synth_minibatch(orc, 700, seed)
    assert np.mean(np.abs(np.exp(mb["old_neglogp"].astype(np.float64) - orc.step(mb["obs"], np.zeros((700, 6), np.float32))[2]) - 1) > 0) > 0.5


def cpu_case(hidden, O, A, n, seed=3):
    """the reference's own chain of a case: (padded parameters, minibatch around the chain's own outputs)"""
    orc = seeded_oracle(hidden, O, A, seed)
    lay = R.Layout(O, A, hidden)
    theta = np.zeros(lay.P_pad, np.float32)
    theta[lay.dense_mask()] = orc.theta
    p = lay.params(theta)
    rng = np.random.RandomState(5)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32); noise = rng.normal(size=(n, A)).astype(np.float32)
    f = R.chain_forward(p, obs, R.rne_bf16, A)
    mu32 = f["mu"].astype(np.float32)
    act = R.act_epilogue(mu32, p["logstd"][:A], noise)[0].astype(np.float32)
    nlp = R.nlp_terms(mu32, p["logstd"][:A], act)[3].astype(np.float32)
    mb = H.synth_minibatch_from(obs, act, f["v"].astype(np.float32), nlp, seed)
    return orc, lay, p, mb


@pytest.mark.parametrize("case", list(CASES))
def test_cpu_emulation_shares_stay_under_the_recorded_figures(case):
    """rule (2) / (3) of tests/bf16_ref.py take their caps from NumPy fp32 arithmetic on the same operands: what that emulation shows on the reference's own
    chain of each case is recorded there (CPU_SHARES, CPU_L2) and must not drift upwards unnoticed"""
    hidden, O, A, n = CASES[case]
    orc, lay, p, mb = cpu_case(hidden, O, A, n)
    sh = R.cpu_chain_shares(p, mb, A, float(np.float32(CR)), orc.cfg.ent_coef, orc.cfg.vf_coef)
    print(case, {k: "%.3g" % v for k, v in sh.items()})
    for k, cap in R.CPU_SHARES.items():
        assert sh[k] <= cap, (k, sh[k], cap)
    for k, cap in R.CPU_L2.items():
        assert sh[k] <= cap, (k, sh[k], cap)


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


def test_comparison_rules_reject_faults_the_old_criteria_accept():
    """With the reference alone (no kernel modified, nothing run on a GPU): the reference's stand-in for a kernel's output is perturbed the way a subtly wrong
    kernel would be, and the comparison functions must reject it -- while the criteria of tests/test_bf16_path.py (per-tensor gradient cosine > 0.995, global
    norm within 3 %, vf_loss within 3 %) accept the first two.
      1. truncation instead of round-to-nearest-even, everywhere
      2. one 64-row stage dropped from one 128 x 128 tile of one weight gradient
      3. bias gradients summed from the rounded values instead of the fp32 ones"""
    hidden, O, A, n = (1024, 512), 64, 18, 512
    orc, lay, p, mb = cpu_case(hidden, O, A, n)
    cr, ent, vfc = float(np.float32(CR)), orc.cfg.ent_coef, orc.cfg.vf_coef
    exact_losses, exact, _ = R.chain_train(p, mb, R.identity, A, cr, cr, 0.0, ent, vfc)           # what the fp32 oracle computes (shown above at 1e-5)
    good_losses, good, im = R.chain_train(p, mb, R.rne_bf16, A, cr, cr, 0.0, ent, vfc)
    names = [k for k in exact if k.endswith("/w") or k.endswith("/b")]
    ref_norm = np.sqrt(sum((exact[k] ** 2).sum() for k in exact))

    def old_criteria(losses, grads):
        norm = np.sqrt(sum((grads[k] ** 2).sum() for k in grads))
        ok = abs(norm / ref_norm - 1) < 3e-2 and abs(losses[1] / exact_losses[1] - 1) < 3e-2
        return ok and all(cosine(grads[k], exact[k]) > 0.995 for k in names if np.linalg.norm(exact[k]) > 1e-3 * ref_norm)
    assert old_criteria(good_losses, good)
    f, Wb = im["f"], im["f"]["Wb"]
    x, w, b = f["h"][0][0], Wb["W"][0][1], p["b"][0][1]
    y, E = R.hidden_forward(x, w, b)
    share_ref = R.mismatch_share(R.emu_hidden_forward(x, w, b), y)
    R.check_bf16("the stand-in itself", R.emu_hidden_forward(x, w, b), y, E, share_ref)
    # 1. truncation
    t_losses, t_grads, _ = R.chain_train(p, mb, R.trunc_bf16, A, cr, cr, 0.0, ent, vfc)
    assert old_criteria(t_losses, t_grads), "the old criteria accept a path that truncates"
    q = R.trunc_bf16(R.emu_tanh_f32(R.f32(x) @ R.f32(w), b))
    with pytest.raises(AssertionError, match="not rne|leave the bracket"):
        R.check_bf16("truncated hidden layer", q, y, E, share_ref)
    assert R.bf16_findings(q, y, E, share_ref)[1] > 0.3
    # 2. a dropped stage of one tile
    xw, dyw = f["h"][0][0], im["dy"][0][1]
    ref, Ew = R.weight_grad(xw, dyw, extra_adds=8)
    emu = R.emu_weight_grad(xw, dyw)
    l2_ref = R.rel_l2(emu, ref)
    R.check_f32("the stand-in itself", emu, ref, Ew, l2_ref)
    bad = emu.copy()
    bad[128:256, 256:384] -= R.emu_weight_grad(xw[64:128, 128:256], dyw[64:128, 256:384])
    d_grads = dict(good); d_grads["pi_fc1/w"] = bad.astype(np.float64)
    assert old_criteria(good_losses, d_grads), "the old criteria accept a weight gradient that lost a stage of one tile"
    with pytest.raises(AssertionError, match="further from the float64 value"):
        R.check_f32("dW with a dropped stage", bad, ref, Ew, l2_ref)
    # 3. bias sums of the rounded values
    d, wh, h1 = im["dhead"][0], Wb["Wh"][0], f["h"][0][1]
    yb, Eb = R.tanh_grad(d, wh, h1)
    sums, Es = R.column_sums(yb, Eb, n)
    e32 = R.emu_tanh_grad_f32(d, wh, h1)
    l2_ref = R.rel_l2(e32.sum(0, dtype=np.float32), sums)
    R.check_f32("the stand-in itself", e32.sum(0, dtype=np.float32), sums, Es, l2_ref)
    with pytest.raises(AssertionError, match="relative L2|further from"):
        R.check_f32("bias sums of the rounded values", R.rne_bf16(e32).sum(0, dtype=np.float32), sums, Es, l2_ref)


# =====================================================================================================================================================
# GPU: one handle per case, an act pass, then a train step, every stage checked
# =====================================================================================================================================================
class Dev:
    """a PPO_BF16 handle with seeded weights and typed reads of its workspaces"""

    def __init__(self, hidden, O, A, seed=3):
        import ppo_cpp_amd
        self.orc = seeded_oracle(hidden, O, A, seed)
        self.g = ppo_cpp_amd.PPOHip(O, A, list(hidden), compute_dtype=BF16)
        self.g.set_flat(self.orc.theta)
        self.lay = R.Layout(O, A, hidden)
        assert [(n, s) for n, _, s in self.orc.tensors] == list(self.g.tensors) and [n for n, _ in self.g.tensors] == self.lay.order
        self.rec = R.Record()

    def f32(self, name):
        return self.g.debug_buffer(name).view(np.float32)

    def bf(self, name, width):
        return R.from_bits(self.g.debug_buffer(name).view(np.uint16)).reshape(-1, width)

    def theta_and_mirror(self):
        """(padded fp32 weights, padded bf16 mirror as fp32) after checking that the mirror IS rne(theta) on every padded element, and that the padded vector
        holds the dense weights where the layout says"""
        lay, g = self.lay, self.g
        th = self.f32("theta")
        assert th.size == lay.P_pad
        np.testing.assert_array_equal(lay.dense(th), g.get_flat(0))
        assert not th[~lay.dense_mask()].any(), "padding weights are zero"
        mir = self.g.debug_buffer("bf_theta").view(np.uint16)
        assert mir.size == lay.P_pad
        np.testing.assert_array_equal(mir, R.bf16_bits(R.rne_bf16(th)), err_msg="theta_bf != rne(theta)")
        return th, R.from_bits(mir)


def check_forward(d, th, mir, n, tag):
    """staged rows -> hidden layers -> head sums, from the device's buffers.  Returns (x0, h[t][l], mu32 [n][A], v32 [n]) as the device holds them"""
    lay, rec = d.lay, d.rec
    Rp = R.ru(n, 128)
    pf, pw = lay.params(th), lay.params(mir)
    x0 = d.bf("bf_x0", lay.Kp0)[:Rp]
    h = [[], []]
    for t, tw in enumerate(("pi", "vf")):
        x = x0
        for l in range(lay.L):
            q = d.bf("bf_h_%s_%d" % (tw, l), lay.Hp[l])[:Rp]
            y, E = R.hidden_forward(x, pw["W"][t][l], pf["b"][t][l])
            share_ref = R.mismatch_share(R.emu_hidden_forward(x, pw["W"][t][l], pf["b"][t][l]), y)
            R.check_bf16("%s hidden forward %s layer %d" % (tag, tw, l), q, y, E, share_ref, rec)
            rec.note("hidden forward", **rec["%s hidden forward %s layer %d" % (tag, tw, l)])
            h[t].append(q); x = q
    sums = []
    for t, tw in enumerate(("pi", "vf")):
        parts = d.f32("bf_head_%s" % tw).reshape(4, -1, lay.Ap)[:, :Rp]
        cols = slice(0, lay.A) if t == 0 else slice(0, 1)
        ref, E = R.heads(h[t][-1], pw["Wh"][t], pf["bh"][t])
        l2_ref = R.rel_l2(R.emu_heads(h[t][-1], pw["Wh"][t], pf["bh"][t])[:, cols], ref[:, cols])
        R.check_f32("%s head sums %s" % (tag, tw), parts.astype(np.float64).sum(0)[:, cols], ref[:, cols], E[:, cols], l2_ref, rec)
        rec.note("head sums", **rec["%s head sums %s" % (tag, tw)])
        assert all(np.abs(parts[k][:, cols]).max() > 0 for k in range(4)), "the handle's head_split is GB_HEAD_SPLIT = 4 for every hidden width (a multiple of 128)"
        sums.append(R.head_sum_f32(parts))
    return x0, h, sums[0][:n, :lay.A], sums[1][:n, 0]


def check_act_pass(d, n, seed, tag="act"):
    """ppo_step on n seeded rows: staging (exact), mirror (exact), hidden layers, heads, the sampling epilogue.  Returns what the train step is built around."""
    lay, g, rec = d.lay, d.g, d.rec
    rng = np.random.RandomState(seed)
    obs = rng.uniform(-1, 1, (n, lay.O)).astype(np.float32); noise = rng.normal(size=(n, lay.A)).astype(np.float32)
    th, mir = d.theta_and_mirror()
    a, v, nlp = g.step(obs, noise)
    Rp = R.ru(n, 128)
    np.testing.assert_array_equal(R.bf16_bits(d.bf("bf_x0", lay.Kp0)[:Rp]), R.bf16_bits(R.stage_obs(obs, Rp, lay.Kp0)), err_msg="x0 != rne(obs), zero padding")
    x0, h, mu32, v32 = check_forward(d, th, mir, n, tag)
    ls = lay.params(th)["logstd"][:lay.A]
    np.testing.assert_array_equal(v, v32, err_msg="value != the head partial products added in range order")
    np.testing.assert_array_equal(g.act_deterministic(obs), mu32)
    R.check_f32(tag + " action", a, *R.act_epilogue(mu32, ls, noise), rec=rec)
    ref_nlp, E_nlp = R.nlp_terms(mu32, ls, a)[3:5]
    R.check_f32(tag + " neglogp", nlp, ref_nlp, E_nlp, rec=rec)
    return dict(obs=obs, a=a, v=v, nlp=nlp, x0=x0, h=h, mu32=mu32, v32=v32)


def check_train_step(d, act, seed, vclip=("policy", 0.0), tag="train"):
    """ppo_train_step on a minibatch built around the handle's own act outputs: loss, backward, weight gradients, assembly, clip + Adam, the new mirror"""
    lay, g, rec = d.lay, d.g, d.rec
    n = act["obs"].shape[0]
    Rp = R.ru(n, 128)
    mode, rng_vf = vclip
    mb = H.synth_minibatch_from(act["obs"], act["a"], act["v"], act["nlp"], seed, vf_ranges=(rng_vf,) if mode == "range" else None)
    th0, mir0 = d.theta_and_mirror()                                   # BEFORE the step: the Adam step rewrites the mirror
    m0, v0, pow0 = d.f32("adam_m").copy(), d.f32("adam_v").copy(), g.beta_powers().copy()
    pf, pw = lay.params(th0), lay.params(mir0)
    losses = g.train_step(LR, CR, mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
    # ---- forward: the same launches on the same rows and weights as the act pass -> the same bits
    np.testing.assert_array_equal(R.bf16_bits(d.bf("bf_x0", lay.Kp0)[:Rp]), R.bf16_bits(act["x0"]), err_msg="train x0")
    h = [[d.bf("bf_h_%s_%d" % (tw, l), lay.Hp[l])[:Rp] for l in range(lay.L)] for tw in ("pi", "vf")]
    for t in range(2):
        for l in range(lay.L):
            np.testing.assert_array_equal(R.bf16_bits(h[t][l]), R.bf16_bits(act["h"][t][l]), err_msg="train h[%d][%d] != act h" % (t, l))
    parts = [d.f32("bf_head_%s" % tw).reshape(4, -1, lay.Ap)[:, :Rp] for tw in ("pi", "vf")]
    mu32, v32 = R.head_sum_f32(parts[0])[:n, :lay.A], R.head_sum_f32(parts[1])[:n, 0]
    np.testing.assert_array_equal(mu32, act["mu32"]); np.testing.assert_array_equal(v32, act["v32"])
    # ---- loss
    cr = float(np.float32(CR))
    vcr, voff = {"policy": (cr, 0.0), "range": (float(np.float32(rng_vf)), 0.0), "off": (0.0, np.inf)}[mode]
    ls = pf["logstd"][:lay.A]
    lo = R.loss(mu32, v32, ls, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"], cr, vcr, voff, g.cfg.ent_coef, g.cfg.vf_coef)
    dmu32, dv32 = R.emu_loss_grads_f32(mu32, v32, ls, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"], cr, vcr, voff, g.cfg.vf_coef)
    dhead = [d.bf("bf_dhead_pi", lay.Ap)[:Rp], d.bf("bf_dhead_vf", lay.Ap)[:Rp]]
    R.check_bf16(tag + " dhead_pi", dhead[0][:n, :lay.A], lo["dmu"], lo["E_dmu"], R.mismatch_share(R.rne_bf16(dmu32), lo["dmu"]), rec)
    R.check_bf16(tag + " dhead_vf", dhead[1][:n, 0], lo["dv"], lo["E_dv"], R.mismatch_share(R.rne_bf16(dv32), lo["dv"]), rec)
    rec.note("dhead", **rec[tag + " dhead_pi"]); rec.note("dhead", **rec[tag + " dhead_vf"])
    assert not dhead[0][n:].any() and not dhead[0][:, lay.A:].any(), "dhead_pi: rows >= n and padding columns are zero"
    assert not dhead[1][n:].any() and not dhead[1][:, 1:].any(), "dhead_vf: only column 0 of rows < n is ever non-zero"
    for k, name in enumerate(("pg_loss", "vf_loss", "entropy", "approxkl", "clipfrac")):
        R.check_f32("%s %s" % (tag, name), losses[k], lo["terms"][k][0], lo["terms"][k][1], rec=rec)
    # ---- backward: every link from the device's own dy / dhead, weights and tanh outputs; bias sums from the fp32 products
    nt = Rp // (256 if Rp % 256 == 0 else 128)
    dbias = d.f32("bf_dbias").reshape(-1, lay.n_dbias)[:nt].astype(np.float64).sum(0)
    dy = [[None] * lay.L, [None] * lay.L]
    bias_ref = {}
    for t, tw in enumerate(("pi", "vf")):
        up = dhead[t]
        for l in range(lay.L - 1, -1, -1):
            w = pw["Wh"][t] if l == lay.L - 1 else pw["W"][t][l + 1]
            q = d.bf("bf_dy_%s_%d" % (tw, l), lay.Hp[l])[:Rp]
            y, E = R.tanh_grad(up, w, h[t][l])
            e32 = R.emu_tanh_grad_f32(up, w, h[t][l])
            nm = "%s backward %s layer %d" % (tag, tw, l)
            R.check_bf16(nm, q, y, E, R.mismatch_share(R.rne_bf16(e32), y), rec)
            rec.note("backward", **rec[nm])
            assert not q[n:].any(), "dy rows >= n are zero"
            sums, Es = R.column_sums(y, E, Rp)
            off = lay.db_off[(t, l)]
            R.check_f32(nm + " bias sums", dbias[off:off + lay.Hp[l]], sums, Es, R.rel_l2(e32.sum(0, dtype=np.float32), sums), rec)
            rec.note("bias sums", **rec[nm + " bias sums"])
            bias_ref["%s_fc%d/b" % (tw, l)] = (sums, Es)
            dy[t][l] = q; up = q
    # ---- weight gradients: the slabs (as many per element as workgroups touched its tile), the assembled gradient, ppo_get_last_grad
    grad = d.f32("grad")[:lay.P_pad].copy()
    slabs = d.f32("slabs").reshape(-1, lay.P_pad)
    cnt = lay.slab_counts(Rp, slabs.shape[0])
    acc32 = np.zeros(lay.P_pad, np.float32); acc64 = np.zeros(lay.P_pad)
    for k in range(int(cnt.max())):
        acc32 = np.where(cnt > k, (acc32 + slabs[k]).astype(np.float32), acc32); acc64 += np.where(cnt > k, slabs[k], 0.0)
    np.testing.assert_array_equal(grad[cnt > 0], acc32[cnt > 0], err_msg="the assembled weight gradients are the slabs added in slab order")
    for t, tw in enumerate(("pi", "vf")):
        for l in range(lay.L + 1):
            name = "%s_fc%d/w" % (tw, l) if l < lay.L else "%s/w" % tw
            x = (h[t][l - 1] if l else act["x0"])
            up = dy[t][l] if l < lay.L else dhead[t]
            ref, E = R.weight_grad(x, up, extra_adds=int(cnt.max()))
            l2_ref = R.rel_l2(R.emu_weight_grad(x, up), ref)
            for src, vec in (("slabs", acc64), ("grad", grad)):
                nm = "%s dW %s (%s)" % (tag, name, src)
                R.check_f32(nm, lay.mat(vec, name), ref, E, l2_ref, rec)
                rec.note("dW", **rec[nm])
    for name, (sums, Es) in bias_ref.items():
        R.check_f32("%s grad %s" % (tag, name), lay.mat(grad, name)[0], sums, Es, rec=rec)
    R.check_f32(tag + " grad pi/b", lay.mat(grad, "pi/b")[0][:lay.A], *lo["db_mu"], rec=rec)
    R.check_f32(tag + " grad pi/logstd", lay.mat(grad, "pi/logstd")[0][:lay.A], *lo["dlogstd"], rec=rec)
    R.check_f32(tag + " grad vf/b", lay.mat(grad, "vf/b")[0][0], *lo["db_v"], rec=rec)
    assert not grad[~lay.dense_mask()].any(), "the gradient of every padding element is zero"
    lg, norm = g.last_grad()
    np.testing.assert_array_equal(lg, lay.dense(grad))
    # ---- clip + Adam from the kernel's own assembled gradient
    ca = R.clip_adam(grad, th0, m0, v0, pow0, LR, g.cfg.max_grad_norm, g.cfg.adam_beta1, g.cfg.adam_beta2, g.cfg.adam_eps)
    R.check_f32(tag + " global norm", norm, ca["norm"], ca["E_norm"], rec=rec)
    m1, v1 = d.f32("adam_m"), d.f32("adam_v")
    R.check_f32(tag + " adam m", m1, ca["m"], ca["E_m"], rec=rec)
    R.check_f32(tag + " adam v", v1, ca["v"], ca["E_v"], rec=rec)
    th1, _ = d.theta_and_mirror()                                     # (the mirror the Adam step wrote is rne(theta) again)
    R.check_f32(tag + " theta", th1, *R.theta_step(th0, m1, v1, ca["alpha"], g.cfg.adam_eps), rec=rec)
    np.testing.assert_array_equal(g.beta_powers(), ca["pow_after"])
    assert np.abs(th1 - th0).max() > 0.5 * LR
    return dict(norm=norm, clipped=norm > g.cfg.max_grad_norm, losses=losses)


def report(d, what):
    print("\n[bf16 stages] %s" % what)
    for k in ("hidden forward", "head sums", "dhead", "backward", "bias sums", "dW"):
        if k in d.rec:
            print("    %-16s %s" % (k, "  ".join("%s=%.3g" % kv for kv in sorted(d.rec[k].items()))))
    worst = {}
    for k, v in d.rec.items():
        if "bound_units" in v and "rel_l2" not in v and k not in ("head sums", "bias sums", "dW"):
            key = " ".join(k.split()[-2:])
            worst[key] = max(worst.get(key, 0.0), v["bound_units"])
    print("    fp32 scalars / vectors, largest |out - ref| in units of the derived bound: " + "  ".join("%s=%.3g" % kv for kv in sorted(worst.items())))


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_every_stage_of_an_act_pass_and_a_train_step(case):
    """One handle per case: ppo_step, then ppo_train_step on a minibatch around the handle's own outputs; every stage against float64 on its own device inputs
    (rules and bounds: tests/bf16_ref.py; the largest figures observed on an MI355X per stage: OBSERVED above)."""
    hidden, O, A, n = CASES[case]
    d = Dev(hidden, O, A)
    act = check_act_pass(d, n, seed=5)
    out = check_train_step(d, act, seed=3)
    report(d, "%s %s: norm %.4g, losses %s" % (case, CASES[case], out["norm"], out["losses"]))
    if case == "tiles256_stage4_chain":
        # ppo_kernel_counts counts the path's SEQUENCES ("bf16_step_sequence", "bf16_train_sequence"), not the launches inside them, so that the chained launch ran
        # cannot be read there.  What can be asserted: the shape qualifies (bf16_chain: 2048 rows = 8 row tiles of 256 per tower = 16 row groups, a multiple of 8, times
        # 4 column tiles = 64 workgroups), and the handle still chains at the end -- ppo_debug_raise_chain_error refuses a handle that does not (one created with
        # PPO_HIP_NO_BF16_CHAIN=1, or one whose chained launch failed and fell back): see the per-layer test below for the other side
        k = d.g.kernel_counts()
        assert k["bf16_step_sequence"] >= 1 and k["bf16_train_sequence"] == 1
        d.g.debug_raise_chain_error()
    d.g.close()


@gpu
def test_per_layer_launches_against_float64(monkeypatch):
    """the shape of the chained launch once more with PPO_HIP_NO_BF16_CHAIN=1: the per-layer kernels (gemm_nt_bf16_kernel<4, .>) against float64 themselves, not only
    against the chain"""
    from ppo_cpp_amd.capi import PPOHipError
    monkeypatch.setenv("PPO_HIP_NO_BF16_CHAIN", "1")
    hidden, O, A, n = CASES["tiles256_stage4_chain"]
    d = Dev(hidden, O, A)
    monkeypatch.delenv("PPO_HIP_NO_BF16_CHAIN")
    act = check_act_pass(d, n, seed=5)
    out = check_train_step(d, act, seed=3)
    report(d, "per-layer launches: norm %.4g" % out["norm"])
    with pytest.raises(PPOHipError, match="does not chain"):
        d.g.debug_raise_chain_error()
    d.g.close()


@gpu
def test_changing_row_counts_on_one_handle():
    """ONE (512, 512) handle, 2048 -> 130 -> 1000 -> 300 -> 2048 rows: every stage of every step.  The workspaces keep the capacity of the largest step, so a smaller
    step runs over buffers that still hold the larger one's rows: rows >= n of dhead and dy must be zero (checked in check_train_step), and the weight gradient is
    compared with the float64 product of THIS step's rows -- anything left of the previous step would be outside the bound."""
    d = Dev((512, 512), 64, 18)
    for it, n in enumerate((2048, 130, 1000, 300, 2048)):
        act = check_act_pass(d, n, seed=50 + it, tag="step %d act" % it)
        out = check_train_step(d, act, seed=60 + it, tag="step %d train" % it)
        Rcap = d.g.debug_buffer("bf_x0").size * 2 // d.lay.Kp0
        assert Rcap == 2048
    report(d, "row counts 2048, 130, 1000, 300, 2048 on one handle")
    d.g.close()


@gpu
@pytest.mark.parametrize("mode,rng_vf", [("policy", 0.0), ("range", R_VF), ("off", 0.0)])
def test_value_clip_modes(mode, rng_vf):
    hidden, O, A, n = CASES["tiles128_ragged_elementwise_staging"]
    d = Dev(hidden, O, A)
    d.g.set_value_clip(mode, rng_vf)
    act = check_act_pass(d, n, seed=5)
    out = check_train_step(d, act, seed=3, vclip=(mode, rng_vf))
    report(d, "value clip %s: vf_loss %.5g" % (mode, out["losses"][1]))
    d.g.close()


@gpu
def test_three_consecutive_train_steps():
    """mirror, Adam slots and beta powers after each of three steps; the clip bites on these inputs (returns perturbed by 0.5: the value tower's gradient is large)"""
    hidden, O, A, n = CASES["tiles128_ragged_elementwise_staging"]
    d = Dev(hidden, O, A)
    clipped = []
    for it in range(3):
        act = check_act_pass(d, n, seed=70 + it, tag="step %d act" % it)
        out = check_train_step(d, act, seed=80 + it, tag="step %d train" % it)
        clipped.append(out["clipped"])
    np.testing.assert_allclose(d.g.beta_powers(), [d.g.cfg.adam_beta1 ** 4, d.g.cfg.adam_beta2 ** 4], rtol=1e-6)
    report(d, "three steps, clipped: %s" % clipped)
    assert all(clipped)
    d.g.close()


@gpu
@pytest.mark.parametrize("O,E", [(18, 300), (256, 200)])
def test_rollout_staging(O, E):
    """The act path normalises while it stages (bf16_stage_kernel for O = 18, bf16_stage4_kernel for O = 256): x0 = rne(the normalised fp32 row), and that fp32 row is
    what the rollout stores.  (a) ppo_rollout_act: bf_x0 == rne(rollout obs of that step), bit for bit, padding zero.  (b) after ppo_collect_synthetic the buffer holds
    the BOOTSTRAP value pass's rows (enqueue_finish restaged it), i.e. the seeded env's observation of step T under the statistics as they stand at the finish: compared
    with that, computed in NumPy fp32 (every operation of the kernel's expression is correctly rounded)."""
    import ppo_cpp_amd
    A, T, hidden = 6, 3, (128,)
    g = ppo_cpp_amd.PPOHip(O, A, list(hidden), compute_dtype=BF16)
    g.init_orthogonal(1)
    lay = R.Layout(O, A, hidden)
    Rp = R.ru(E, 128)

    def x0():
        return R.from_bits(g.debug_buffer("bf_x0").view(np.uint16)).reshape(-1, lay.Kp0)[:Rp]
    g.norm_init(E, GAMMA); g.rollout_alloc(E, T)
    g.collect_synthetic(77, GAMMA, LAM, None)
    mean, var, _ = g.norm_stats(0)
    raw, _, _ = o.seeded_env_step(77, 0, E, T, O)
    want = R.normalise_f32(raw, mean, var, 1e-8, 10.0)
    np.testing.assert_array_equal(R.bf16_bits(x0()), R.bf16_bits(R.stage_obs(want, Rp, lay.Kp0)), err_msg="x0 after the bootstrap pass")
    assert np.abs(want).max() > 0.5 and np.mean(R.rne_bf16(want) != want) > 0.5          # (the rounding is not vacuous)
    # (a) a rollout step of a host Env: the staged rows are the rounded stored rows
    rng = np.random.RandomState(2)
    g.rollout_reset(rng.normal(size=(E, O)).astype(np.float32) * 3 + 1)
    g.rollout_act(0, rng.normal(size=(E, A)).astype(np.float32))
    g.sync()
    stored = g.rollout_get("obs")[0]
    np.testing.assert_array_equal(R.bf16_bits(x0()), R.bf16_bits(R.stage_obs(stored, Rp, lay.Kp0)), err_msg="x0 of a rollout step")
    assert np.abs(stored).max() > 0.5
    g.close()
