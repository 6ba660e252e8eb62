"""The wide categorical head of the bf16 path: PPO_ACT_CATEGORICAL | PPO_ACT_BF16_HEAD | PPO_ACT_BF16_WIDE_HEAD with compute_dtype PPO_BF16, 128 < act_dim <= 1024
(bf16_logits_kernel, bf16_value_head_kernel, bf16_{sample,loss,eval}_wide_kernel<EPT, MASK>; include/ppo_hip.h).  In the manner of tests/test_bf16_stages.py and
tests/test_bf16_categorical.py every stage is fed the DEVICE's own inputs and compared with float64.

Tolerances are derived, never read from the device (tests/bf16_wide_ref.py): bf16_cat_ref's derivation with the summation path EPT + 6 additions in the place of its
7.  For logits whose spread stays within 20 that is under 2e-5 absolute on neglogp and under 1e-4 on the entropy at A = 1024; the inputs (init_random(9), pi_gain 1)
keep the device's logits within that spread, which the stage test asserts, with the two figures.  The logits are compared with the float64 product of the device's
own bf16 H_L and bf16 weights plus the fp32 bias under 2 K U sum|h||w|, the bound bf16_ref applies to an fp32-accumulated bf16 product of depth K.
Near-ties of the perturbed logits: none may be left out at these row counts; the float64 reference chain is asserted to have none before any device output is read.

    case     O   hidden     A     rows  what it hits
    A129     7   (40,)      129   24    first column past the old limit, the second 128-column block holds one column; EPT 4, most elements absent; A odd
    A321     11  (136, 72)  321   130   Ap = 384: three column tiles; EPT 8, a ragged last element; rows cross a 128-row tile, dead rows behind them
    A1024    5   (64,)      1024  20    the limit, no padding; EPT 16; the loss kernel's LDS opt-in
"""
import numpy as np
import pytest

from tests import bf16_cat_ref as C
from tests import bf16_ref as R
from tests import bf16_wide_ref as W
from tests import counter_draws_ref as D
from tests.masked_categorical_ref import MaskedCatRef

gpu = pytest.mark.gpu
CR, LR, ENT = 0.16102319955825806, 0.000393141177482903, 0.01
CASES = {"A129": (7, (40,), 129, 24), "A321": (11, (136, 72), 321, 130), "A1024": (5, (64,), 1024, 20)}
WIDE = 0x10000
both = pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])


def inputs(O, A, n, masked, seed=7):
    """observations, uniforms and a mask: about half the categories forbidden, category 3 forbidden in every row, every row with an allowed one"""
    rng = np.random.RandomState(seed)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    mask = (rng.uniform(size=(n, A)) < 0.5).astype(np.float32)
    mask[:, 3] = 0.0
    mask[mask.sum(1) == 0, 0] = 1.0
    return obs, u, (mask if masked else None)


class Dev:
    def __init__(self, case, wide=True, **kw):
        import ppo_cpp_amd
        self.O, self.hidden, self.A, self.n = CASES[case]
        self.ref = MaskedCatRef(self.O, self.A, self.hidden, ent_coef=ENT)
        self.ref.init_random(9, 1.0)
        self.g = ppo_cpp_amd.PPOHip(self.O, self.A, list(self.hidden), action_dist="categorical", compute_dtype=1, bf16_head=True, bf16_wide_head=wide, ent_coef=ENT, **kw)
        self.g.set_flat(self.ref.theta.astype(np.float32))
        self.lay = R.Layout(self.O, self.A, self.hidden)

    def logits_values(self, n):
        """the device's own fp32 logits ([1][Rcap][Ap], unsplit) and values (the 128-column image's partial products added in range order)"""
        lg = self.g.debug_buffer("bf_head_pi").view(np.float32).reshape(-1, self.lay.Ap)
        vp = self.g.debug_buffer("bf_head_vf").view(np.float32).reshape(4, -1, 128)
        return lg[:n, :self.A].copy(), R.head_sum_f32(vp)[:n, 0]

    def bf(self, name, width):
        return R.from_bits(self.g.debug_buffer(name).view(np.uint16)).reshape(-1, width)


def chain_logits(d, obs):
    """the float64 reference's logits on bf16-rounded operands (the CPU side of the near-tie assertions)"""
    spec = dict((name, d.ref.t(name)) for name, _ in d.ref.specs)
    L = len(d.hidden)
    p = dict(W=[[spec["%s_fc%d/w" % (t, l)] for l in range(L)] for t in ("pi", "vf")], b=[[spec["%s_fc%d/b" % (t, l)] for l in range(L)] for t in ("pi", "vf")],
             Wh=[spec["pi/w"], spec["vf/w"]], bh=[spec["pi/b"], spec["vf/b"]])
    return R.chain_forward(p, obs, R.rne_bf16, d.A)["mu"]


def names(masked):
    sfx = "<wcat,mask>" if masked else "<wcat>"
    return "bf16_step_sequence" + sfx, "bf16_train_sequence" + sfx


@gpu
@both
@pytest.mark.parametrize("case", list(CASES))
def test_stages_against_float64_from_the_devices_own_inputs(case, masked):
    d = Dev(case)
    g, lay, n, A = d.g, d.lay, d.n, d.A
    obs, u, mk = inputs(d.O, A, n, masked)
    assert not C.tie_rows(*C.perturbed(chain_logits(d, obs), u, mk)).any(), "the seed leaves no near-tie row in the float64 reference"
    mir, th = R.from_bits(g.debug_buffer("bf_theta").view(np.uint16)), g.debug_buffer("theta").view(np.float32)
    a, v, nlp = g.step(obs, u, mask=mk)
    lg, v32 = d.logits_values(n)
    # ---- logits: the float64 product of the device's own bf16 H_L and bf16 weights + the fp32 bias
    Rp, K = R.ru(n, 128), lay.Hp[-1]
    hL = d.bf("bf_h_pi_%d" % (lay.L - 1), K)[:Rp]
    z, s = R.affine(hL, lay.mat(mir, "pi/w"), lay.mat(th, "pi/b")[0])
    full = g.debug_buffer("bf_head_pi").view(np.float32).reshape(-1, lay.Ap)[:Rp]
    R.check_f32("logits", full, z, 2 * K * R.U * s)
    assert lg.max() - lg.min() <= 20.0, "the inputs keep the logit spread within 20"
    # ---- act: action, deterministic action, neglogp, value from the device's own logits; no row may be left out
    assert C.check_sampled("action", a, lg, u, mk, max_skip=0.0) == 0
    want, E = W.nlp_bound(lg, a, mk)
    assert E.max() < 2e-5
    R.check_f32("neglogp", nlp, want, E)
    np.testing.assert_array_equal(v, v32)
    C.check_det("deterministic action", g.act_deterministic(obs, mask=mk), lg, mk)
    # ---- train: d logits (as bf16), exact zeros, slot column sums, loss terms
    mb = C.synth_batch_from(obs, a, v, nlp, 3, CR)
    losses = g.train_step(LR, CR, mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"], mask=mk)
    lg2, v2 = d.logits_values(n)
    np.testing.assert_array_equal(lg2, lg); np.testing.assert_array_equal(v2, v32)
    cr = float(np.float32(CR))
    lo = W.loss(lg, v32, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"], cr, ENT, g.cfg.vf_coef, mk)
    assert lo["E_H"].max() < 1e-4
    emu = C.emu_loss_dlogits_f32(lg, mb["actions"], mb["advs"], mb["old_neglogp"], CR, ENT, mk)
    q = d.bf("bf_dhead_pi", lay.Ap)[:Rp]
    C.check_dlogits("d logits", q[:n, :A], lo, R.mismatch_share(R.rne_bf16(emu)[lo["ok"]], lo["dl"][lo["ok"]]))
    for part in (q[n:], q[:, A:], q[:n, :A][~lo["ok"]]):
        assert not part.any() and not np.signbit(part).any(), "dead rows, padding columns and forbidden categories are exactly +0"
    slots = g.debug_buffer("slots_pi").view(np.float32).reshape(-1, 2 * lay.Ap + 8)[:Rp // 16]
    assert not slots[:, lay.Ap:2 * lay.Ap].any(), "the aux slot words are zeros"
    np.testing.assert_array_equal(slots[:, A:lay.Ap], 0.0)
    R.check_f32("slot column sums", slots[:, :A].astype(np.float64).sum(0), lo["db"][0], lo["db"][1] + 2 * len(slots) * R.U * np.abs(lo["dl"]).sum(0))
    for k, name in enumerate(("pg_loss", "vf_loss", "entropy", "approxkl", "clipfrac")):
        R.check_f32(name, losses[k], *lo["terms"][k])
    st, tr = names(masked)
    assert g.kernel_count(st) == 2 and g.kernel_count(tr) == 1 and g.kernel_count("bf16_step_sequence<cat>") == 0 and g.kernel_count("bf16_step_sequence<cat,mask>") == 0
    g.close()


@gpu
@both
@pytest.mark.parametrize("case", list(CASES))
def test_one_neglogp_in_three_places(case, masked):
    """ppo_step's neglogp, the train model's (approxkl == 0, clipfrac == 0 on the step's own outputs) and ppo_evaluate_actions' are the same bits; so is the value"""
    d = Dev(case)
    obs, u, mk = inputs(d.O, d.A, d.n, masked)
    a, v, nlp = d.g.step(obs, u, mask=mk)
    d.g.set_bf16_queries(True)
    ev_v, ev_nlp, ev_ent = d.g.evaluate_actions(obs, a, mask=mk)
    np.testing.assert_array_equal(ev_nlp, nlp); np.testing.assert_array_equal(ev_v, v)
    assert np.isfinite(ev_ent).all() and ev_ent.min() > 0
    p = d.g.action_probability(obs, mask=mk)
    assert p.shape == (d.n, d.A) and np.allclose(p.sum(1), 1.0, atol=1e-5)
    if masked:
        assert not p[mk == 0].any() and not np.signbit(p[mk == 0]).any()
    losses = d.g.train_step(LR, CR, obs, a, np.linspace(-1, 1, d.n).astype(np.float32), v + 0.3, nlp, v, mask=mk)
    assert losses[3] == 0.0 and losses[4] == 0.0 and np.isfinite(losses).all(), losses
    d.g.close()


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_all_ones_mask_gives_the_unmasked_bits(case):
    d0, d1 = Dev(case), Dev(case)
    obs, u, _ = inputs(d0.O, d0.A, d0.n, False)
    ones = np.ones((d0.n, d0.A), np.float32)
    a, v, nlp = d0.g.step(obs, u)
    for x, y in zip((a, v, nlp), d1.g.step(obs, u, mask=ones)):
        np.testing.assert_array_equal(x, y)
    mb = C.synth_batch_from(obs, a, v, nlp, 11, CR)
    args = (mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
    np.testing.assert_array_equal(d0.g.train_step(LR, CR, *args), d1.g.train_step(LR, CR, *args, mask=ones))
    np.testing.assert_array_equal(d0.g.last_grad()[0], d1.g.last_grad()[0])
    for which in range(3):
        np.testing.assert_array_equal(d0.g.get_flat(which), d1.g.get_flat(which))
    d0.g.close(); d1.g.close()


@gpu
@both
@pytest.mark.parametrize("case", ["A129", "A321"])
def test_gradient_of_one_train_step_against_the_float64_reference(case, masked):
    """tests/test_bf16_categorical.py's test of this name at the wide shapes: cosine > 0.995 per tensor that carries more than 1e-3 of the norm, the global norm
    within 3 %; category 3, forbidden in every row, gets an exactly zero pi/w column and pi/b entry; the logstd region of theta and both Adam slots never moves"""
    d = Dev(case)
    obs, u, mk = inputs(d.O, d.A, d.n, masked)
    a, v, nlp, _ = d.ref.step(obs, u, mk)
    mb = C.synth_batch_from(obs, a, v.astype(np.float32), nlp.astype(np.float32), 3, CR)
    args = (mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
    _, ref_grad = d.ref.loss_grad(*args, CR, mk)
    off = d.lay.t["pi/logstd"][0]
    before = [d.g.debug_buffer(k)[off:off + d.lay.Ap].copy() for k in ("theta", "adam_m", "adam_v")]
    d.g.train_step(LR, CR, *args, mask=mk)
    grad, norm = d.g.last_grad()
    ref_norm = np.sqrt(ref_grad @ ref_grad)
    assert norm == pytest.approx(ref_norm, rel=3e-2)
    for name, (o, shape) in d.ref.offs.items():
        gt, rt = grad[o:o + int(np.prod(shape))], ref_grad[o:o + int(np.prod(shape))]
        if np.linalg.norm(rt) > 1e-3 * ref_norm:
            c = float(gt.astype(np.float64) @ rt / (np.linalg.norm(gt) * np.linalg.norm(rt)))
            assert c > 0.995, (name, c)
    if masked:
        (ow, sw), (ob, _) = d.ref.offs["pi/w"], d.ref.offs["pi/b"]
        gw = grad[ow:ow + sw[0] * sw[1]].reshape(sw)
        assert np.all(gw[:, 3] == 0.0) and grad[ob + 3] == 0.0 and np.any(gw[:, 4] != 0.0)
    for k, b in zip(("theta", "adam_m", "adam_v"), before):
        np.testing.assert_array_equal(d.g.debug_buffer(k)[off:off + d.lay.Ap], b, err_msg="padded logstd region of " + k)
    d.g.close()


@gpu
@both
def test_on_device_draws_past_column_127(masked):
    """noise = NULL: the action is the argmax built from counter_draws_ref's uniforms for j in [0, A)"""
    d = Dev("A321")
    obs, _, mk = inputs(d.O, d.A, d.n, masked)
    seed = 11
    u = D.counter_uniforms(D.seed_key(seed), np.arange(d.n), 0, d.A).astype(np.float32)
    assert not C.tie_rows(*C.perturbed(chain_logits(d, obs), u, mk)).any()
    d.g.seed(seed)
    a = d.g.step(obs, mask=mk)[0]
    assert C.check_sampled("seeded action", a, d.logits_values(d.n)[0], u, mk, max_skip=0.0) == 0
    d.g.close()


def run_update(monkeypatch, switch):
    for s in ("PPO_HIP_NO_BF16_CHAIN", "PPO_HIP_NO_REDUCE_ADAM"):
        monkeypatch.delenv(s, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    E, T = 64, 8
    d = Dev("A321")
    d.g.set_action_masking(True)
    d.g.norm_init(E, 0.99); d.g.rollout_alloc(E, T)
    d.g.collect_synthetic(5, 0.99, 0.95, None)
    rng = np.random.RandomState(2)
    perms = np.stack([rng.permutation(E * T) for _ in range(2)]).astype(np.int32)
    rows = d.g.update(LR, CR, 2, 4, perms)[0]
    out = [rows] + [d.g.get_flat(w) for w in range(3)]
    # (the synthetic collect's steps carry no mask rows: they count under the plain step name; the update trains under the rollout's masks)
    nodes, counts = d.g.debug_graph_nodes(), [d.g.kernel_count(names(False)[0]) + d.g.kernel_count(names(True)[0]), d.g.kernel_count(names(True)[1])]
    d.g.close()
    return out, nodes, counts


@gpu
def test_update_and_launch_forms(monkeypatch):
    """ppo_update on a device-env rollout at A321 (E = 64, T = 8, 4 minibatches): kernel nodes only, finite losses, the new names count; PPO_HIP_NO_BF16_CHAIN=1 and
    PPO_HIP_NO_REDUCE_ADAM=1 give the default form's bits"""
    want, nodes, counts = run_update(monkeypatch, None)
    assert np.isfinite(want[0]).all() and counts[0] > 0 and counts[1] > 0, counts
    assert nodes is not None and nodes["kernel"] > 0 and nodes["memset"] == 0 and nodes["memcpy"] == 0 and nodes["other"] == 0, nodes
    for switch in ("PPO_HIP_NO_BF16_CHAIN", "PPO_HIP_NO_REDUCE_ADAM"):
        for x, y in zip(want, run_update(monkeypatch, switch)[0]):
            np.testing.assert_array_equal(x, y, err_msg=switch)


def test_create_refusals_flag_and_names():
    """parse_create answers before any HIP call: no GPU needed"""
    import ctypes
    import os
    import ppo_cpp_amd
    from ppo_cpp_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "#define PPO_ACT_BF16_WIDE_HEAD 0x10000" in open(os.path.join(root, "include", "ppo_hip.h")).read() and capi.ACT_BF16_WIDE_HEAD == WIDE
    lib = ppo_cpp_amd.load_library()
    h = ctypes.c_void_p()

    def create(A, dist, dtype=1):
        cfg = capi.PPOConfig()
        lib.ppo_config_default(ctypes.byref(cfg), 7, A, 1, (ctypes.c_int32 * 1)(40))
        cfg.compute_dtype = dtype
        assert lib.ppo_create_ex(ctypes.byref(cfg), dist, ctypes.byref(h)) != 0
        return cfg, lib.ppo_last_error(None).decode()
    msg = create(1025, 1 | 0x200 | WIDE)[1]
    assert "PPO_ACT_BF16_WIDE_HEAD" in msg and "1024" in msg and "1025" in msg, msg
    assert create(129, 1 | 0x200)[1] == "ppo_create_ex: PPO_ACT_BF16_HEAD: the categorical head of the PPO_BF16 path holds at most 128 categories (got 129)"
    msg = create(6, 3 | WIDE, 0)[1]
    assert "unknown action_dist" in msg and "PPO_ACT_BF16_WIDE_HEAD" in msg, msg
    cfg = create(6, 3 | WIDE, 0)[0]
    assert lib.ppo_create_multi_ex(ctypes.byref(cfg), (ctypes.c_int32 * 2)(3, 3), 2, WIDE, ctypes.byref(h)) != 0
    assert "unknown flag bit 0x10000" in lib.ppo_last_error(None).decode()
    with pytest.raises(ValueError, match="bf16_wide_head"):
        ppo_cpp_amd.PPOHip(7, 6, [40], action_dist="multi_binary", bf16_wide_head=True)
    variants = [lib.ppo_kernel_variant_name(i).decode() for i in range(200) if lib.ppo_kernel_variant_name(i)]
    for masked in (False, True):
        for name in names(masked):
            assert name in variants and len(name) < 32, name                # the char[32] rows callers copy a variant name into
