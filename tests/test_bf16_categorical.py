"""The categorical head (and action masks) of the bf16 matrix-core path: a handle created with PPO_ACT_CATEGORICAL | PPO_ACT_BF16_HEAD and compute_dtype PPO_BF16
(include/ppo_hip.h).  The GEMMs around the head are the Gaussian handle's and are checked stage by stage in tests/test_bf16_stages.py; here the two kernels that hold
the head's arithmetic (bf16_sample_kernel / bf16_loss_kernel<cat[,mask]>) are fed the DEVICE's own logits -- the head GEMM's partial products ("bf_head_pi") added in
range order, bf16_ref.head_sum_f32 -- and compared with float64 under bounds derived from the fp32 operations (tests/bf16_cat_ref.py, where every bound is derived).
Bitwise properties (all-ones mask == unmasked, act model == train model, chained == per-layer, one-launch assembly == two launches) and end-to-end runs against the
library's fp32 categorical handle follow.

Inputs of the stage checks: weights CatRef.init_random(9, pi_gain=1.0), observations and uniforms RandomState(7), masks random_masks(RandomState(3), n, A).  With
these the float64 reference has no row whose two best perturbed logits are closer than 1e-4 at any of the five shapes (smallest gap 3.7e-4), so no row should have
to be left out as a near-tie; the tests print how many were.

OBSERVED on an MI355X (largest over every GPU test of this module; units: the share of the derived bound an element needed, 1.0 is the edge): see OBSERVED below.
"""
import numpy as np
import pytest

from tests import bf16_cat_ref as C
from tests import bf16_ref as R
from tests.categorical_ref import CatRef
from tests.masked_categorical_ref import MaskedCatRef, random_masks

gpu = pytest.mark.gpu

CR = 0.16102319955825806
LR = 0.000393141177482903
GAMMA, LAM = 0.99, 0.95
BF16 = 1
ENT = 0.01            # the entropy coefficient of the train checks: large enough for a dropped entropy term to leave the bracket of a bf16 d logit

# (hidden, O, A, n): the smallest shapes that reach each way the two kernels can go wrong
CASES = {
    "A6_ragged_tile_dead_rows": ((256, 128), 18, 6, 130),           # A < 16; a ragged last 128-row tile; dead rows in a loss block
    "A70_second_element_padding": ((1280,), 18, 70, 128),           # a lane's second element (j >= 64); head ranges of one and a quarter image; 70 < Ap
    "A128_no_padding": ((128,), 7, 128, 64),                        # A == Ap: no padding column, both elements of every lane live
    "A2_minimum": ((128,), 7, 2, 64),
    "A18_chain_stage4": ((512, 512), 64, 18, 2048),                 # chained launches; stage4 staging behind the non-16-byte gather
}

# twice the largest mismatch share of rne(fp32 emulation of d logits) against rne(float64) over the five CASES, masked and unmasked, on the reference's own chain
# (test_cpu_emulation_share_stays_under_the_recorded_figure; measured 0 .. 1.2e-3: the d logits of a row are few and of one magnitude, like d mu)
CPU_SHARES = {"dlogits": 2.5e-3}

OBSERVED = """
    stage / output                 units of E     share q != rne(y) (its cap in that case)
    d logits (bf_dhead_pi)         0.054          4.9e-4 (1.2e-3) at (128,) / 7 / 128 / 64; 1.5e-4 (5.2e-4) at 2048 x 18 masked; 0 of 780 at A = 6
    neglogp (act)                  0.39           (collect_synthetic: see that test's print)
    value                          0              (the range-order sum itself)
    pi/b gradient (slot sums)      0.058
    pg_loss / vf_loss / entropy / approxkl / clipfrac   0.0059 / 0.0057 / 0.0093 / 0.034 / 0.0033
    rows left out as fp32 near-ties of the perturbed logits: 0 in every case (allowed: n // 256)
    update against the fp32 categorical handle: entropy rows differ by 7.7e-5 (allowance 3.3e-4 = 10 x the reference's own 3.3e-5) at 64 x 8 / 4 and by 3.5e-5
    (allowance 1.6e-4) at 100 x 10 / 5; host layer: reward curve first-15 0.088, last-15 0.444
"""


def make_ref(hidden, O, A, ent_coef=ENT, seed=9, pi_gain=1.0):
    ref = MaskedCatRef(O, A, hidden, ent_coef=ent_coef)
    ref.init_random(seed, pi_gain)
    return ref


def inputs(O, A, n):
    rng = np.random.RandomState(7)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    return obs, u, random_masks(np.random.RandomState(3), n, A)


def ref_batch(ref, obs, u, mask, seed=3):
    """a minibatch around the float64 reference's own outputs (CPU tests)"""
    a, v, nlp, _ = ref.step(obs, u, mask)
    return C.synth_batch_from(obs, a, v.astype(np.float32), nlp.astype(np.float32), seed, CR)


# =====================================================================================================================================================
# CPU: the reference and its comparison rules
# =====================================================================================================================================================
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("hidden,O,A,n", [((24, 16), 11, 6, 40), ((40,), 7, 70, 24)])
def test_head_reference_agrees_with_the_categorical_references(hidden, O, A, n, masked):
    """the float64 head reference of tests/bf16_cat_ref.py, fed EXACT logits, against CatRef / MaskedCatRef (step, and loss_grad by torch autograd) at 1e-9: actions,
    neglogp, the five loss terms, and the d logits -- as the pi/b gradient (their column sums), the pi/w gradient (h^T d logits) and, row by row, the pi/b gradient
    of one-row minibatches (a row's d logits themselves)"""
    ref = make_ref(hidden, O, A)
    obs, u, mask = inputs(O, A, n)
    mk = mask if masked else None
    logits, v = ref.forward(obs)
    ra, rv, rnlp, pert = ref.step(obs, u, mk)
    hd = C.head(logits, mk)
    np.testing.assert_array_equal(C.argmax_lowest(C.perturbed(logits, u, mk)[0]), ra)
    np.testing.assert_allclose(hd["nlp_all"][np.arange(n), ra], rnlp, rtol=1e-9, atol=1e-9)
    if masked:
        np.testing.assert_array_equal(C.argmax_lowest(np.where(mask != 0, logits, -np.inf)), ref.act_deterministic(obs, mask))
    mb = ref_batch(ref, obs, u, mk)
    args = (mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
    ref_losses, ref_grad = ref.loss_grad(*args, CR, mk)
    lo = C.loss(logits, v, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"], CR, CR, 0.0, ref.ent, ref.vfc, mk, exact_consts=True)
    np.testing.assert_allclose([t[0] for t in lo["terms"]], ref_losses, rtol=1e-9, atol=1e-9)
    hp = np.asarray(obs, np.float64)
    for l in range(len(hidden)):
        hp = np.tanh(hp @ ref.t("pi_fc%d/w" % l) + ref.t("pi_fc%d/b" % l))
    np.testing.assert_allclose(lo["db"][0], ref.t("pi/b", ref_grad), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(hp.T @ lo["dl"], ref.t("pi/w", ref_grad), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(lo["db_v"][0], ref.t("vf/b", ref_grad)[0], rtol=1e-9, atol=1e-9)
    assert np.abs(lo["dl"]).max() > 1e-3
    for i in (0, 1, n - 1):                                     # one-row minibatches: the pi/b gradient IS the row's d logits (g = 1)
        one = [x[i:i + 1] for x in args]
        _, g1 = ref.loss_grad(*one, CR, None if mk is None else mk[i:i + 1])
        lo1 = C.loss(logits[i:i + 1], v[i:i + 1], one[1], one[2], one[3], one[5], one[4], CR, CR, 0.0, ref.ent, ref.vfc, None if mk is None else mk[i:i + 1], exact_consts=True)
        np.testing.assert_allclose(lo1["dl"][0], ref.t("pi/b", g1), rtol=1e-9, atol=1e-9)


def cpu_case(case, masked):
    """the reference's own bf16 chain of a case: logits and values as fp32, a minibatch around the chain's own outputs"""
    hidden, O, A, n = CASES[case]
    ref = make_ref(hidden, O, A)
    obs, u, mask = inputs(O, A, n)
    mk = mask if masked else None
    spec = dict((name, ref.t(name)) for name, _ in ref.specs)
    L = len(hidden)
    p = dict(W=[[spec["%s_fc%d/w" % (t, l)] for l in range(L)] for t in ("pi", "vf")], b=[[spec["%s_fc%d/b" % (t, l)] for l in range(L)] for t in ("pi", "vf")],
             Wh=[spec["pi/w"], spec["vf/w"]], bh=[spec["pi/b"], spec["vf/b"]])
    f = R.chain_forward(p, obs, R.rne_bf16, A)
    lg, v = f["mu"].astype(np.float32), f["v"].astype(np.float32)
    a = C.argmax_lowest(C.perturbed(lg, u, mk)[0])
    nlp = C.head(lg, mk)["nlp_all"][np.arange(n), a]
    mb = C.synth_batch_from(obs, a, v, nlp.astype(np.float32), 3, CR)
    return ref, p, obs, u, mk, lg, v, mb


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_cpu_emulation_share_stays_under_the_recorded_figure(case, masked):
    """rule (2) takes its cap from NumPy fp32 arithmetic on the same logits: what that emulation shows on the reference's own chain is recorded (CPU_SHARES)"""
    ref, p, obs, u, mk, lg, v, mb = cpu_case(case, masked)
    lo = C.loss(lg, v, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"], float(np.float32(CR)), float(np.float32(CR)), 0.0, ref.ent, ref.vfc, mk)
    emu = C.emu_loss_dlogits_f32(lg, mb["actions"], mb["advs"], mb["old_neglogp"], CR, ref.ent, mk)
    ok = lo["ok"]
    share = R.mismatch_share(R.rne_bf16(emu)[ok], lo["dl"][ok])
    print(case, "masked" if masked else "plain", "share %.3g of %d" % (share, ok.sum()))
    assert share <= CPU_SHARES["dlogits"], share
    C.check_dlogits("the emulation itself", R.rne_bf16(emu), lo, share)


def test_comparison_rules_reject_planted_faults():
    """on the reference's own data (nothing runs on a GPU): the stand-in for a kernel's output is perturbed the way a wrong kernel would be, and the functions the
    GPU tests call must reject it
      1. a non-zero d logit on a forbidden category        2. the entropy term of d logits dropped
      3. the normaliser summed over forbidden categories   4. a tie resolved to the higher index"""
    ref, p, obs, u, mk, lg, v, mb = cpu_case("A6_ragged_tile_dead_rows", True)
    n, A = lg.shape
    cr = float(np.float32(CR))
    lo = C.loss(lg, v, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"], cr, cr, 0.0, ref.ent, ref.vfc, mk)
    emu = C.emu_loss_dlogits_f32(lg, mb["actions"], mb["advs"], mb["old_neglogp"], CR, ref.ent, mk)
    share = R.mismatch_share(R.rne_bf16(emu)[lo["ok"]], lo["dl"][lo["ok"]])
    good = R.rne_bf16(emu)
    C.check_dlogits("the stand-in itself", good, lo, share)
    R.check_f32("the stand-in's pi/b sums", emu.sum(0, dtype=np.float32), *lo["db"])
    # 1.
    bad = good.copy()
    i, j = np.argwhere(~lo["ok"])[0]
    bad[i, j] = np.float32(2.0 ** -20)
    with pytest.raises(AssertionError, match="forbidden"):
        C.check_dlogits("a forbidden category with a gradient", bad, lo, share)
    # 2.
    dropped = C.emu_loss_dlogits_f32(lg, mb["actions"], mb["advs"], mb["old_neglogp"], CR, ref.ent, mk, drop_entropy=True)
    with pytest.raises(AssertionError, match="not rne|leave the bracket"):
        C.check_dlogits("d logits without the entropy term", R.rne_bf16(dropped), lo, share)
    with pytest.raises(AssertionError, match="further from the float64 value"):
        R.check_f32("pi/b sums without the entropy term", dropped.sum(0, dtype=np.float32), *lo["db"])
    # 3.
    a = mb["actions"].astype(np.int64)
    nlp_good = C.head(lg, mk)["nlp_all"][np.arange(n), a].astype(np.float32)
    C.check_nlp("the stand-in itself", nlp_good, lg, a, mk)
    m = np.where(mk != 0, lg.astype(np.float64), -np.inf).max(1, keepdims=True)
    z_all = np.exp(lg - m).sum(1)                                   # every category in the sum, the maximum still the allowed one
    nlp_bad = (np.log(z_all) - (lg[np.arange(n), a] - m[:, 0])).astype(np.float32)
    with pytest.raises(AssertionError, match="further from the float64 value"):
        C.check_nlp("normaliser over the forbidden categories too", nlp_bad, lg, a, mk)
    # 4.  two equal logits (and equal uniforms): the rule is the lowest index
    tie = lg.copy(); ut = u.copy()
    lowi = np.argmax(mk[5] != 0); highi = A - 1 - np.argmax(mk[5][::-1] != 0)
    mk2 = mk.copy(); mk2[5] = 0; mk2[5, [0, A - 1]] = 1
    tie[5, 0] = tie[5, A - 1] = np.float32(0.75); ut[5, 0] = ut[5, A - 1] = np.float32(0.5)
    det = C.argmax_lowest(np.where(mk2 != 0, tie.astype(np.float64), -np.inf)).astype(np.float32)
    smp = C.argmax_lowest(C.perturbed(tie, ut, mk2)[0]).astype(np.float32)
    assert det[5] == 0 and smp[5] == 0 and lowi <= highi
    C.check_det("the stand-in itself", det, tie, mk2); C.check_sampled("the stand-in itself", smp, tie, ut, mk2)
    det_bad, smp_bad = det.copy(), smp.copy()
    det_bad[5] = smp_bad[5] = A - 1
    with pytest.raises(AssertionError, match="lowest-index argmax"):
        C.check_det("tie to the higher index", det_bad, tie, mk2)
    with pytest.raises(AssertionError, match="differ from the float64 Gumbel argmax"):
        C.check_sampled("tie to the higher index", smp_bad, tie, ut, mk2)


def test_flag_is_declared_with_its_value_and_the_names_fit():
    import inspect
    import os
    import ppo_cpp_amd
    from ppo_cpp_amd import capi, hostapi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "ppo_hip.h")).read()
    assert "#define PPO_ACT_BF16_HEAD 0x200" in src and "#define PPO_ABI_VERSION 3" in src
    assert capi.ACT_BF16_HEAD == 0x200
    assert inspect.signature(ppo_cpp_amd.PPOHip.__init__).parameters["bf16_head"].default is False
    assert inspect.signature(hostapi.learn_curve).parameters["compute_dtype"].default == 0
    assert inspect.signature(hostapi.learn_masked).parameters["compute_dtype"].default == 0
    hip = open(os.path.join(root, "ppo_cpp_amd", "csrc", "ppo_hip.hip")).read()
    for name in ("bf16_step_sequence<cat>", "bf16_step_sequence<cat,mask>", "bf16_train_sequence<cat>", "bf16_train_sequence<cat,mask>"):
        assert len(name) < 32 and '"%s"' % name in hip          # ppo_kernel_counts' char[32]


# =====================================================================================================================================================
# GPU
# =====================================================================================================================================================
class Dev:
    """a categorical PPO_BF16 handle with the reference's weights and typed reads of its workspaces"""

    def __init__(self, hidden, O, A, ent_coef=ENT, seed=9, pi_gain=1.0, masking=False, **kw):
        import ppo_cpp_amd
        self.ref = make_ref(hidden, O, A, ent_coef, seed, pi_gain)
        self.g = ppo_cpp_amd.PPOHip(O, A, list(hidden), action_dist="categorical", compute_dtype=BF16, bf16_head=True, ent_coef=ent_coef, **kw)
        assert list(self.g.tensors) == [(n, s) for n, s in self.ref.specs], "4L + 4 tensors, no pi/logstd"
        self.g.set_flat(self.ref.theta.astype(np.float32))
        if masking:
            self.g.set_action_masking(True)
        self.lay = R.Layout(O, A, hidden)                      # (the padded vector keeps the logstd slot: the Gaussian layout's offsets hold)
        self.O, self.A = O, A
        self.rec = R.Record()

    def f32(self, name):
        return self.g.debug_buffer(name).view(np.float32)

    def bf(self, name, width):
        return R.from_bits(self.g.debug_buffer(name).view(np.uint16)).reshape(-1, width)

    def logits_values(self, n):
        """the device's own logits / values of the last pass: the head's partial products added in range order"""
        Rp = R.ru(n, 128)
        lp = self.f32("bf_head_pi").reshape(4, -1, self.lay.Ap)[:, :Rp]
        vp = self.f32("bf_head_vf").reshape(4, -1, self.lay.Ap)[:, :Rp]
        return R.head_sum_f32(lp)[:n, :self.A], R.head_sum_f32(vp)[:n, 0]

    def close(self):
        self.g.close()


def report(d, what):
    print("\n[bf16 categorical] %s" % what)
    for k, v in sorted(d.rec.items()):
        print("    %-34s %s" % (k, "  ".join("%s=%.3g" % kv for kv in sorted(v.items()))))


def check_act(d, obs, u, mk, tag):
    g, n = d.g, obs.shape[0]
    a, v, nlp = g.step(obs, u, mask=mk)
    lg, v32 = d.logits_values(n)
    C.check_sampled(tag + " action", a, lg, u, mk)
    C.check_nlp(tag + " neglogp", nlp, lg, a, mk, d.rec)
    R.check_f32(tag + " value", v, v32, 0.0, rec=d.rec)           # (the value IS the range-order sum: bound 0)
    det = g.act_deterministic(obs, mask=mk)
    C.check_det(tag + " deterministic action", det, d.logits_values(n)[0], mk)
    np.testing.assert_array_equal(d.logits_values(n)[0], lg, err_msg="the deterministic pass leaves the same logits")
    if mk is not None:
        assert np.all(mk[np.arange(n), a.astype(np.int64)] != 0) and np.all(mk[np.arange(n), det.astype(np.int64)] != 0)
        g.seed(3)
        a2 = g.step(obs, mask=mk)[0]                               # the counter draw under the mask
        assert np.all(mk[np.arange(n), a2.astype(np.int64)] != 0)
    return a, v, nlp


def check_train(d, obs, a, v, nlp, mk, tag, seed=3, floor=0.0, normal=0.0):
    """floor, normal: bf16_cat_ref.check_dlogits' underflow floor (added to every bound here, once per summed row for the pi/b sums) and the size from which a d logit
    counts in the rounding share; 0 and 0 for logits of order 1"""
    g, lay, rec = d.g, d.lay, d.rec
    n, A = obs.shape[0], d.A
    Rp = R.ru(n, 128)
    mb = C.synth_batch_from(obs, a, v, nlp, seed, CR)
    losses = g.train_step(LR, CR, mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"], mask=mk)
    lg, v32 = d.logits_values(n)
    cr = float(np.float32(CR))
    lo = C.loss(lg, v32, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"], cr, cr, 0.0, g.cfg.ent_coef, g.cfg.vf_coef, mk)
    emu = C.emu_loss_dlogits_f32(lg, mb["actions"], mb["advs"], mb["old_neglogp"], CR, g.cfg.ent_coef, mk)
    q = d.bf("bf_dhead_pi", lay.Ap)[:Rp]
    sel = C.normal_size(lo, normal)
    C.check_dlogits(tag + " d logits", q[:n, :A], lo, R.mismatch_share(R.rne_bf16(emu)[sel], lo["dl"][sel]) if sel.any() else 0.0, rec, floor, normal)
    assert not q[n:].any() and not q[:, A:].any(), "dhead_pi: rows >= n and padding columns are zero"
    assert not np.signbit(q[:n, :A][~lo["ok"]]).any() and not np.signbit(q[:, A:]).any(), "forbidden and padding columns are +0"
    for k, name in enumerate(("pg_loss", "vf_loss", "entropy", "approxkl", "clipfrac")):
        R.check_f32("%s %s" % (tag, name), losses[k], lo["terms"][k][0], lo["terms"][k][1] + floor, rec=rec)
    slots = d.f32("slots_pi").reshape(-1, 2 * lay.Ap + 8)[:Rp // 16]
    assert not slots[:, lay.Ap:2 * lay.Ap].any(), "the aux (d logstd) slot words are zeros"
    grad, norm = g.last_grad()
    ob, _ = d.ref.offs["pi/b"]
    R.check_f32(tag + " grad pi/b", grad[ob:ob + A], lo["db"][0], lo["db"][1] + n * floor, rec=rec)
    np.testing.assert_array_equal(slots[:, :lay.Ap].astype(np.float64).sum(0)[A:], 0.0)
    return mb, lo, losses, grad


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("case", list(CASES))
def test_head_stages_from_the_devices_own_logits(case, masked):
    """ppo_step, ppo_act_deterministic and ppo_train_step at the five shapes, masked and unmasked: action, deterministic action, neglogp, value from the device's own
    logits; d logits (bracket, exact-rounding share, exact zeros), the pi/b gradient, the loss terms and the aux slot words from the train pass's own logits"""
    hidden, O, A, n = CASES[case]
    d = Dev(hidden, O, A)
    obs, u, mask = inputs(O, A, n)
    mk = mask if masked else None
    a, v, nlp = check_act(d, obs, u, mk, "act")
    check_train(d, obs, a, v, nlp, mk, "train")
    kc = d.g.kernel_counts()
    sfx = "<cat,mask>" if masked else "<cat>"
    other = "<cat>" if masked else "<cat,mask>"
    assert kc["bf16_step_sequence" + sfx] >= 2 and kc["bf16_train_sequence" + sfx] == 1, kc
    assert kc["bf16_step_sequence" + other] == 0 and kc["bf16_train_sequence" + other] == 0 and kc["bf16_step_sequence"] == 0 and kc["bf16_train_sequence"] == 0, kc
    assert kc["policy_step_kernel<cat>"] == 0 and kc["train_fwd_bwd_kernel<cat>"] == 0, kc
    report(d, "%s %s %s" % (case, CASES[case], "masked" if masked else "plain"))
    d.close()


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("case", ["A6_ragged_tile_dead_rows", "A70_second_element_padding", "A128_no_padding"])
def test_act_model_and_train_model_give_the_same_neglogp_bits(case, masked):
    """old_neglogp = step(..)[2] on the same rows, actions and weights: the first train step's ratio is exactly 1 (approxkl == 0.0, clipfrac == 0.0) -- the
    sample and the loss kernel share their reduction shape (cat_row_norm / cat_row_pick)"""
    hidden, O, A, n = CASES[case]
    d = Dev(hidden, O, A)
    obs, u, mask = inputs(O, A, n)
    mk = mask if masked else None
    a, v, nlp = d.g.step(obs, u, mask=mk)
    rng = np.random.RandomState(1)
    adv = rng.normal(size=n).astype(np.float32)
    losses = d.g.train_step(LR, CR, obs, a, adv, (v + rng.normal(scale=0.5, size=n)).astype(np.float32), nlp, v, mask=mk)
    assert losses[3] == 0.0 and losses[4] == 0.0, losses
    assert np.isfinite(losses).all() and losses[2] > 0
    d.close()


@gpu
def test_a_category_forbidden_everywhere_gets_exact_zeros_and_the_logstd_slot_never_moves():
    hidden, O, A, n = CASES["A6_ragged_tile_dead_rows"]
    dead = 4
    d = Dev(hidden, O, A)
    lay = d.lay
    off, _, _, prow, pcol = lay.t["pi/logstd"]                    # the padded slot a categorical handle keeps without a tensor
    before = [d.g.debug_buffer(k)[off:off + 256].copy() for k in ("theta", "adam_m", "adam_v")]
    assert d.g.debug_buffer("theta").size == lay.P_pad
    ow, sw = d.ref.offs["pi/w"]; ob, _ = d.ref.offs["pi/b"]
    for it in range(3):
        rng = np.random.RandomState(20 + it)
        obs = rng.uniform(-1, 1, (n, O)).astype(np.float32); u = rng.uniform(size=(n, A)).astype(np.float32)
        mask = random_masks(np.random.RandomState(200 + it), n, A, special=False)
        mask[:, dead] = 0.0
        mask[mask.sum(1) == 0, 0] = 1.0
        a, v, nlp = d.g.step(obs, u, mask=mask)
        assert not np.any(a == dead)
        mb = C.synth_batch_from(obs, a, v, nlp, 30 + it, CR)
        d.g.train_step(LR, CR, mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"], mask=mask)
        grad, _ = d.g.last_grad()
        gw = grad[ow:ow + sw[0] * sw[1]].reshape(sw)
        assert np.all(gw[:, dead] == 0.0) and grad[ob + dead] == 0.0, "the forbidden category's pi/w column and pi/b entry get an exactly zero gradient"
        assert np.any(gw[:, dead - 1] != 0.0) and grad[ob + dead - 1] != 0.0
    for k, b in zip(("theta", "adam_m", "adam_v"), before):
        np.testing.assert_array_equal(d.g.debug_buffer(k)[off:off + 256], b, err_msg="padded logstd region of " + k)
        assert not b.any()
    d.close()


def upload(g, fields):
    for f, x in fields.items():
        g.rollout_set(f, np.asarray(x, np.float32))


def ref_fields(ref, rng, E, T, masks=None):
    """an uploaded rollout built by the reference: the actions are consistent with the masks"""
    O, A = ref.O, ref.A
    obs = rng.uniform(-1, 1, (T, E, O)).astype(np.float32)
    a, v, nlp, _ = ref.step(obs.reshape(-1, O), rng.uniform(size=(T * E, A)), None if masks is None else masks.reshape(T * E, A))
    f = {"obs": obs, "actions": a.reshape(T, E), "values": v.reshape(T, E), "neglogp": nlp.reshape(T, E) + rng.normal(scale=0.1, size=(T, E)),
         "dones": (rng.uniform(size=(T, E)) < 0.02).astype(np.float32), "rewards": rng.normal(size=(T, E)),
         "returns": v.reshape(T, E) + rng.normal(scale=0.5, size=(T, E))}
    if masks is not None:
        f["masks"] = masks
    return f


@gpu
def test_all_ones_masks_give_the_unmasked_bits():
    hidden, O, A, n = (256, 128), 18, 18, 130
    E, T, nmb, epochs = 32, 8, 2, 2
    d0, d1 = Dev(hidden, O, A), Dev(hidden, O, A, masking=True)
    g0, g1 = d0.g, d1.g
    obs, u, _ = inputs(O, A, n)
    ones = np.ones((n, A), np.float32)
    for x, y in zip(g0.step(obs, u), g1.step(obs, u, mask=ones)):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(g0.act_deterministic(obs), g1.act_deterministic(obs, mask=ones))
    for it in range(3):
        a, v, nlp = g0.step(obs, u)
        mb = C.synth_batch_from(obs, a, v, nlp, 11 + it, CR)
        args = (mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
        np.testing.assert_array_equal(g0.train_step(LR, CR, *args), g1.train_step(LR, CR, *args, mask=ones))
        for x, y in zip(g0.last_grad(), g1.last_grad()):
            np.testing.assert_array_equal(x, y)
        for which in range(3):
            np.testing.assert_array_equal(g0.get_flat(which), g1.get_flat(which))
    for g in (g0, g1):
        g.norm_init(E); g.rollout_alloc(E, T)
    np.testing.assert_array_equal(g1.rollout_get("masks"), np.ones((T, E, A), np.float32))
    rng = np.random.RandomState(5)
    fields = ref_fields(d0.ref, rng, E, T)
    perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
    out = []
    for g in (g0, g1):
        upload(g, fields)
        out.append(g.update(LR, CR, epochs, nmb, perms))
    np.testing.assert_array_equal(out[0][0], out[1][0]); np.testing.assert_array_equal(out[0][1], out[1][1])
    for which in range(3):
        np.testing.assert_array_equal(g0.get_flat(which), g1.get_flat(which))
    k0, k1 = g0.kernel_counts(), g1.kernel_counts()
    assert k0["bf16_step_sequence<cat>"] > 0 and k0["bf16_train_sequence<cat>"] > 0 and k0["bf16_step_sequence<cat,mask>"] == 0 and k0["bf16_train_sequence<cat,mask>"] == 0, k0
    assert k1["bf16_step_sequence<cat,mask>"] > 0 and k1["bf16_train_sequence<cat,mask>"] > 0 and k1["bf16_step_sequence<cat>"] == 0 and k1["bf16_train_sequence<cat>"] == 0, k1
    for k in (k0, k1):
        assert k["bf16_step_sequence"] == 0 and k["bf16_train_sequence"] == 0, k
    d0.close(); d1.close()


def run_steps(d, obs, u, mk, steps=2):
    out = []
    for it in range(steps):
        a, v, nlp = d.g.step(obs, u, mask=mk)
        mb = C.synth_batch_from(obs, a, v, nlp, 40 + it, CR)
        losses = d.g.train_step(LR, CR, mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"], mask=mk)
        out += [a, v, nlp, losses, d.g.last_grad()[0]] + [d.g.get_flat(w) for w in range(3)]
    return out


@gpu
@pytest.mark.parametrize("switch", ["PPO_HIP_NO_BF16_CHAIN", "PPO_HIP_NO_REDUCE_ADAM"])
def test_launch_forms_agree_bitwise_with_the_categorical_head_in_between(switch, monkeypatch):
    """the chained launch against a launch per layer, and the one-launch assembly + clip + Adam against the two launches, at the 2048-row shape, masked"""
    hidden, O, A, n = CASES["A18_chain_stage4"]
    obs, u, mask = inputs(O, A, n)
    monkeypatch.delenv(switch, raising=False)
    d = Dev(hidden, O, A)
    want = run_steps(d, obs, u, mask)
    if switch == "PPO_HIP_NO_BF16_CHAIN":
        d.g.debug_raise_chain_error()                          # (refused by a handle that does not chain: this one did)
    d.close()
    monkeypatch.setenv(switch, "1")
    d = Dev(hidden, O, A)
    got = run_steps(d, obs, u, mask)                           # (PPO_HIP_NO_REDUCE_ADAM is read again when a step is enqueued)
    monkeypatch.delenv(switch)
    for x, y in zip(want, got):
        np.testing.assert_array_equal(x, y)
    kc = d.g.kernel_counts()
    assert kc["bf16_train_sequence<cat,mask>"] == 2 and (kc["bf16_reduce_adam_kernel"] == 0) == (switch == "PPO_HIP_NO_REDUCE_ADAM"), kc
    d.close()


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


def reference_entropy_deviation(ref, obs_rows, masks_rows, idx_per_mb):
    """what bf16 operands do to a minibatch's mean entropy IN THE REFERENCE: CatRef on the fp32 weights against the same head formulas on
    bf16_ref.chain_forward(.., rne_bf16, ..) logits; the largest |difference| over the given minibatches"""
    spec = dict((name, ref.t(name)) for name, _ in ref.specs)
    L = len(ref.hidden)
    p = dict(W=[[spec["%s_fc%d/w" % (t, l)] for l in range(L)] for t in ("pi", "vf")], b=[[spec["%s_fc%d/b" % (t, l)] for l in range(L)] for t in ("pi", "vf")],
             Wh=[spec["pi/w"], spec["vf/w"]], bh=[spec["pi/b"], spec["vf/b"]])
    exact = C.head(ref.forward(obs_rows)[0], masks_rows)["H"]
    rounded = C.head(R.chain_forward(p, obs_rows, R.rne_bf16, ref.A)["mu"], masks_rows)["H"]
    return max(abs(exact[i].mean() - rounded[i].mean()) for i in idx_per_mb), float(np.abs(exact - rounded).mean())


@gpu
@pytest.mark.parametrize("E,T,nmb", [(64, 8, 4), (100, 10, 5)])
def test_update_tracks_the_fp32_categorical_handle(E, T, nmb):
    """the same uploaded rollout (built by the reference under masks), the same explicit permutations, two epochs at (256, 128) / 18 / 18: the bf16 handle against the
    library's fp32 categorical handle under tests/test_bf16_path.py's tolerances.  128-row minibatches: the epoch is staged once; 200-row ones: each by itself.
    Entropy: a categorical entropy depends on the logits, so the Gaussian test's 1e-4 does not carry over; the allowance is RATE_FACTOR x the deviation the REFERENCE
    shows between fp32 and rne_bf16-chain logits on the first epoch's minibatches (printed; measured on the CPU: 3.3e-5 at 64 x 8 / 4, 1.6e-5 at 100 x 10 / 5,
    i.e. allowances of 3.3e-4 / 1.6e-4 on entropies of ~1.2; observed on an MI355X: 7.7e-5 / 3.5e-5)."""
    import ppo_cpp_amd
    hidden, O, A, epochs = (256, 128), 18, 18, 2
    db = Dev(hidden, O, A, masking=True)
    gf = ppo_cpp_amd.PPOHip(O, A, list(hidden), action_dist="categorical", ent_coef=ENT)
    gf.set_flat(db.ref.theta.astype(np.float32)); gf.set_action_masking(True)
    rng = np.random.RandomState(9)
    masks = random_masks(rng, T * E, A, special=False).reshape(T, E, A)
    fields = ref_fields(db.ref, rng, E, T, masks)
    perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
    rows = {}
    for name, g in (("f32", gf), ("bf16", db.g)):
        g.norm_init(E, GAMMA); g.rollout_alloc(E, T)
        upload(g, fields)
        rows[name] = g.update(LR, CR, epochs, nmb, perms)[0]
    rb, rf = rows["bf16"], rows["f32"]
    # the reference's own deviation on the first epoch's minibatches (env-major rows e * T + t, perms[ep][i] = destination of row i)
    B, M = E * T, E * T // nmb
    flat = lambda x: np.swapaxes(np.asarray(x), 0, 1).reshape((B,) + np.asarray(x).shape[2:])
    inv = np.empty(B, np.int64); inv[perms[0]] = np.arange(B)
    dev_mb, dev_rows = reference_entropy_deviation(db.ref, flat(fields["obs"]), flat(masks), [inv[k * M:(k + 1) * M] for k in range(nmb)])
    allow = R.RATE_FACTOR * dev_mb
    print("entropy: reference deviation per minibatch %.3g (per row %.3g), allowance %.3g, observed %.3g" % (dev_mb, dev_rows, allow, np.abs(rb[:, 2] - rf[:, 2]).max()))
    np.testing.assert_allclose(rb[:, 2], rf[:, 2], rtol=0, atol=allow, err_msg="entropy")
    np.testing.assert_allclose(rb[:, 1], rf[:, 1], rtol=2e-2, err_msg="vf_loss")
    np.testing.assert_allclose(rb[:, 0], rf[:, 0], atol=1e-2, err_msg="pg_loss")
    np.testing.assert_allclose(rb[:, 3], rf[:, 3], rtol=1e-2, atol=2e-3, err_msg="approxkl")
    np.testing.assert_allclose(rb[:, 4], rf[:, 4], atol=0.06, err_msg="clipfrac")
    th0 = db.ref.theta.astype(np.float32)
    assert cosine(db.g.get_flat(0) - th0, gf.get_flat(0) - th0) > 0.9
    nodes = db.g.debug_graph_nodes()
    assert nodes is not None and nodes["kernel"] > 0 and nodes["memset"] == 0 and nodes["memcpy"] == 0 and nodes["other"] == 0, nodes
    kc = db.g.kernel_counts()
    assert kc["bf16_train_sequence<cat,mask>"] > 0 and kc["bf16_train_sequence<cat>"] == 0 and kc["bf16_train_sequence"] == 0 and kc["train_fwd_bwd_kernel<cat,mask>"] == 0, kc
    db.close(); gf.close()


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("case", ["A6_ragged_tile_dead_rows", "A70_second_element_padding"])
def test_gradient_of_one_train_step_against_the_float64_reference(case, masked):
    """against CatRef / MaskedCatRef.loss_grad (torch float64 autograd on the fp32 weights): cosine > 0.995 per tensor that carries more than 1e-3 of the norm, global
    norm within 3 % (tests/test_bf16_path.py's criteria)"""
    hidden, O, A, n = CASES[case]
    d = Dev(hidden, O, A)
    obs, u, mask = inputs(O, A, n)
    mk = mask if masked else None
    mb = ref_batch(d.ref, obs, u, mk)
    args = (mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
    ref_losses, ref_grad = d.ref.loss_grad(*args, CR, mk)
    losses = d.g.train_step(LR, CR, *args, mask=mk)
    grad, norm = d.g.last_grad()
    ref_norm = np.sqrt(ref_grad @ ref_grad)
    assert norm == pytest.approx(ref_norm, rel=3e-2)
    for name, (off, shape) in d.ref.offs.items():
        cnt = int(np.prod(shape))
        gt, rt = grad[off:off + cnt], ref_grad[off:off + cnt]
        if np.linalg.norm(rt) > 1e-3 * ref_norm:
            assert cosine(gt, rt) > 0.995, (name, cosine(gt, rt))
    assert losses[1] == pytest.approx(ref_losses[1], rel=3e-2) and losses[0] == pytest.approx(ref_losses[0], abs=1e-2)
    d.close()


@gpu
def test_collect_synthetic_on_the_device_env():
    """E = 64, T = 4, seeded on-device uniforms: integer actions in [0, A); every stored neglogp is the reference neglogp of the stored action from the logits a fresh
    step leaves for the stored (normalised) observation, within the stage check's bound; one seed twice agrees bitwise, another seed differs"""
    hidden, O, A = (256, 128), 18, 6
    E, T = 64, 4
    d = Dev(hidden, O, A)
    g = d.g
    runs = []
    for seed in (77, 77, 78):                                 # (the collect's draws are keyed by its own seed argument, like the seeded env's)
        g.norm_init(E, GAMMA); g.rollout_alloc(E, T)
        g.collect_synthetic(seed, GAMMA, LAM, None)
        runs.append({f: g.rollout_get(f) for f in ("obs", "actions", "values", "neglogp", "returns")})
    for f in runs[0]:
        np.testing.assert_array_equal(runs[0][f], runs[1][f], err_msg=f)
    assert np.mean(runs[0]["actions"] != runs[2]["actions"]) > 0.3
    ro = runs[2]
    acts = ro["actions"].reshape(-1)
    assert np.all(acts == np.floor(acts)) and acts.min() >= 0 and acts.max() < A and len(np.unique(acts)) > 1
    obs = ro["obs"].reshape(T * E, O)
    v = g.value(obs)                                           # a fresh pass over the stored observations (no normalisation: they are stored normalised)
    lg, v32 = d.logits_values(T * E)
    C.check_nlp("collect neglogp", ro["neglogp"].reshape(-1), lg, acts, None, d.rec)
    np.testing.assert_array_equal(ro["values"].reshape(-1), v32)
    np.testing.assert_array_equal(v, v32)
    report(d, "collect_synthetic")
    kc = g.kernel_counts()
    assert kc["bf16_step_sequence<cat>"] > 0 and kc["bf16_step_sequence"] == 0 and kc["policy_step_kernel<cat>"] == 0, kc
    d.close()


@gpu
def test_on_device_sampling_follows_the_softmax_of_the_devices_logits():
    """65536 copies of one observation, (128,) / 7 / 6, pi_gain 3: seeded frequencies within 4 sigma of the softmax of the device's own logits of row 0"""
    hidden, O, A, n = (128,), 7, 6, 65536
    d = Dev(hidden, O, A, pi_gain=3.0)
    obs = np.tile(np.random.RandomState(2).uniform(-1, 1, (1, O)).astype(np.float32), (n, 1))
    d.g.seed(11)
    a, _, nlp = d.g.step(obs)
    lg, _ = d.logits_values(n)
    assert np.all(lg == lg[0])
    p = C.head(lg[:1])["p"][0]
    assert p.max() < 0.9 and p.min() > 1e-3, p
    freq = np.bincount(a.astype(np.int64), minlength=A) / n
    sigma = np.sqrt(p * (1 - p) / n)
    assert np.all(np.abs(freq - p) <= 4 * sigma), (freq, p, sigma)
    d.g.seed(11)
    np.testing.assert_array_equal(d.g.step(obs)[0], a)
    d.g.seed(12)
    assert np.any(d.g.step(obs)[0] != a)
    d.close()


@gpu
def test_ppo2_learns_the_discrete_target_task_on_the_bf16_path():
    """tests/test_discrete_policy.test_ppo2_learns_the_discrete_target_task with compute_dtype=1: the host shim ORs PPO_ACT_BF16_HEAD into PPO2::action_dist_for for
    a discrete Env.  The same RISE / BAND / reference figure (derived there from the NumPy reference loop).  Measured on an MI355X: first-15 0.088, last-15 0.444."""
    from ppo_cpp_amd import hostapi
    RISE, BAND, REF_LAST15 = 0.20, 0.10, 0.425
    got = hostapi.learn_curve(16, 64, [64, 64], 150, 4, 4, 2e-3, 0.2, seed=11, act_dim=18, discrete=True, compute_dtype=1)
    kc = got["kernel_counts"]
    assert kc["bf16_step_sequence<cat>"] > 0 and kc["bf16_train_sequence<cat>"] > 0 and kc["policy_step_kernel<cat>"] == 0 and kc["bf16_step_sequence"] == 0, kc
    c = got["reward_curve"]
    first, last = c[:15].mean(), c[-15:].mean()
    print("reward curve first-15 %.3f last-15 %.3f" % (first, last))
    assert last - first >= RISE, (first, last)
    assert abs(last - REF_LAST15) <= BAND, (last, REF_LAST15)


@gpu
def test_errors_and_flag_contract():
    import ppo_cpp_amd
    Err = ppo_cpp_amd.PPOHipError
    O, A, hidden, n = 18, 6, [256, 128], 40
    with pytest.raises(Err, match="PPO_BF16"):
        ppo_cpp_amd.PPOHip(O, A, hidden, action_dist="categorical", compute_dtype=1)
    with pytest.raises(Err, match="128"):
        ppo_cpp_amd.PPOHip(O, 129, hidden, action_dist="categorical", compute_dtype=1, bf16_head=True)
    lib = ppo_cpp_amd.load_library()
    import ctypes
    h = ctypes.c_void_p()
    probe = ppo_cpp_amd.PPOHip(O, A, hidden)
    assert lib.ppo_create_ex(ctypes.byref(probe.cfg), 2 | 0x200, ctypes.byref(h)) != 0 and b"unknown action_dist" in lib.ppo_last_error(None)
    probe.close()
    obs, u, mask = inputs(O, A, n)
    ref = make_ref(hidden, O, A)

    def trace(g, noise):
        g.set_flat(np.random.RandomState(1).normal(scale=0.1, size=g.P).astype(np.float32))
        a, v, nlp = g.step(obs, noise)
        losses = g.train_step(LR, CR, obs, a, np.linspace(-1, 1, n).astype(np.float32), v + 0.3, nlp + 0.05, v - 0.1)
        out = [a, v, nlp, losses, g.get_flat(0), g.kernel_counts(), g.lib.ppo_action_dist(g.h)]
        g.close()
        return out
    # the flag on a PPO_F32 categorical handle and on a Gaussian PPO_BF16 handle: the bits and the counts of a handle without it
    for kw, noise in ((dict(action_dist="categorical"), u), (dict(compute_dtype=1), np.random.RandomState(4).normal(size=(n, A)).astype(np.float32))):
        x, y = trace(ppo_cpp_amd.PPOHip(O, A, hidden, **kw), noise), trace(ppo_cpp_amd.PPOHip(O, A, hidden, bf16_head=True, **kw), noise)
        for p, q in zip(x[:5], y[:5]):
            np.testing.assert_array_equal(p, q)
        assert x[5] == y[5] and x[6] == y[6] == (1 if "action_dist" in kw else 0), (x[5], y[5])
    # masks on a Gaussian bf16 handle stay refused
    bf = ppo_cpp_amd.PPOHip(O, A, hidden, compute_dtype=1, bf16_head=True)
    with pytest.raises(Err, match="categorical"):
        bf.step(obs, mask=mask)
    with pytest.raises(Err, match="categorical"):
        bf.set_action_masking(True)
    bf.close()
    # PPO_ACT_SHAPE_KERNELS beside the flag: accepted, the handle is a bf16 one
    g = ppo_cpp_amd.PPOHip(O, A, hidden, action_dist="categorical", compute_dtype=1, bf16_head=True, shape_kernels=True)
    g.step(obs)
    assert g.kernel_counts()["bf16_step_sequence<cat>"] == 1 and g.lib.ppo_action_dist(g.h) == 1
    g.close()
    # data parallel: refused with the documented message, and the handle then still trains
    g = ppo_cpp_amd.PPOHip(O, A, hidden, action_dist="categorical", compute_dtype=1, bf16_head=True)
    g.set_flat(ref.theta.astype(np.float32))
    with pytest.raises(Err, match="data parallel is not supported for a categorical PPO_BF16 handle created with PPO_ACT_BF16_HEAD"):
        g.dist_init(1, 0, b"\0" * 128)
    a, v, nlp = g.step(obs, u, mask=mask)
    theta = g.get_flat(0)
    # host-side refusals before anything is trained: a row without an allowed category, an action its own mask forbids
    none = mask.copy(); none[3] = 0
    with pytest.raises(Err, match="allows no category"):
        g.step(obs, u, mask=none)
    with pytest.raises(Err, match="allows no category"):
        g.train_step(LR, CR, obs, a, v, v, nlp, v, mask=none)
    forb = mask.copy(); forb[2, int(a[2])] = 0; forb[2, (int(a[2]) + 1) % A] = 1
    with pytest.raises(Err, match="forbidden by the row's own mask"):
        g.train_step(LR, CR, obs, a, v, v, nlp, v, mask=forb)
    np.testing.assert_array_equal(g.get_flat(0), theta)
    assert g.kernel_counts()["bf16_train_sequence<cat,mask>"] == 0
    losses = g.train_step(LR, CR, obs, a, np.linspace(-1, 1, n).astype(np.float32), v + 0.3, nlp, v, mask=mask)
    assert np.isfinite(losses).all() and np.any(g.get_flat(0) != theta)
    g.close()
