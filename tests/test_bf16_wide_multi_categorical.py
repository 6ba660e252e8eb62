"""The wide multi-categorical head of the bf16 path: ppo_create_multi_ex with PPO_ACT_BF16_MULTI_HEAD | PPO_ACT_BF16_WIDE_MULTI_HEAD, PPO_BF16, 128 < sum(nvec) <= 1024
(bf16_logits_kernel, bf16_value_head_kernel, bf16_{sample,loss,eval}_wide_multi_kernel<EPT, MASK>; include/ppo_hip.h).  Every stage is fed the DEVICE's own inputs
and compared with float64, as tests/test_bf16_wide_categorical.py does, with that file's inputs: init_random(9, 1.0), RandomState(7), about half the categories
forbidden, column 3 forbidden in every row; a component whose mask came out all zero gets its first category allowed.

Tolerances are derived, never read from the device: tests/bf16_mcat_ref.py's per-component composition (row totals in component order, bounds added) over
tests/bf16_wide_ref.py's summation path -- a component's sums take EPT + 6 additions, EPT that of the whole ROW (widened(), below).
No (row, component) pair may be left out as a near-tie: the float64 chain is asserted to have none (0 of 72, 520 and 320 pairs) before any device output is read.

    case    O   hidden     nvec                  rows  what it hits
    M129    7   (40,)      (2, 125, 2)           24    first width past the old limit, EPT 4; a component crossing the 128-column tile; the last one in an almost empty block
    M321    11  (136, 72)  (5, 251, 2, 63)       130   Ap 384, EPT 8; a component ending on the 256-column quad boundary; two components in one lane's quad (256..259);
                                                       rows cross a 128-row tile, dead rows behind
    M1024   5   (64,)      (2,)*8 + (126,)*8     20    the limit, no padding, EPT 16; K = 16: four full batches; two components per quad
"""
import ctypes
import os
import types

import numpy as np
import pytest

from tests import bf16_cat_ref as C
from tests import bf16_mcat_ref as M
from tests import bf16_ref as R
from tests import bf16_wide_ref as W
from tests.multi_categorical_ref import MultiCatRef

gpu = pytest.mark.gpu
CR, LR, ENT = 0.16102319955825806, 0.000393141177482903, 0.01
CASES = {"M129": (7, (40,), (2, 125, 2), 24), "M321": (11, (136, 72), (5, 251, 2, 63), 130), "M1024": (5, (64,), (2,) * 8 + (126,) * 8, 20)}
WIDEM, MULTI = 0x20000, 0x1000
both = pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
cases = pytest.mark.parametrize("case", list(CASES))


def inputs(O, nvec, n, masked):
    A = int(sum(nvec))
    rng = np.random.RandomState(7)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    mask = (rng.uniform(size=(n, A)) < 0.5).astype(np.float32)
    mask[:, 3] = 0.0
    for o, e in M.comps(nvec):
        mask[mask[:, o:e].sum(1) == 0, o] = 1.0
    return obs, u, (mask if masked else None)


def widened(monkeypatch, A):
    """bf16_mcat_ref composing bf16_wide_ref's bounds instead of bf16_cat_ref's: every component sum is charged the row's EPT + 6 additions, whatever its own width"""
    ept = W.ept_of(A)
    monkeypatch.setattr(W, "ept_of", lambda _: ept)
    ns = types.SimpleNamespace(**vars(C))
    ns.nlp_bound = lambda hd, ai: (C.nlp_bound(hd, ai)[0] + (ept - 1) * W.U,)
    ns.loss = lambda lg, v, a, adv, ret, ov, onlp, cr, vcr, voff, ent, vf, mask=None, exact_consts=False: W.loss(lg, v, a, adv, ret, ov, onlp, cr, ent, vf, mask)
    monkeypatch.setattr(M, "C", ns)


class Dev:
    def __init__(self, case, wide=True, nvec=None, **kw):
        import ppo_cpp_amd
        self.O, self.hidden, nv, self.n = CASES[case]
        self.nvec = tuple(nvec or nv)
        self.A = int(sum(self.nvec))
        self.ref = MultiCatRef(self.O, self.nvec, self.hidden, ent_coef=ENT)
        self.ref.init_random(9, 1.0)
        self.g = ppo_cpp_amd.PPOHip(self.O, None, list(self.hidden), action_dist="multi_categorical", nvec=list(self.nvec), compute_dtype=1, bf16_head=True,
                                    multi_bf16_wide_head=wide, ent_coef=ENT, **kw)
        self.g.set_flat(self.ref.theta.astype(np.float32))
        self.lay = R.Layout(self.O, self.A, self.hidden)

    def logits_values(self, n):
        """the device's own fp32 logits ([1][Rcap][Ap], unsplit) and values (the 128-column image's partial products added in range order)"""
        lg = self.g.debug_buffer("bf_head_pi").view(np.float32).reshape(-1, self.lay.Ap)
        vp = self.g.debug_buffer("bf_head_vf").view(np.float32).reshape(4, -1, 128)
        return lg[:n, :self.A].copy(), R.head_sum_f32(vp)[:n, 0]

    def bf(self, name, width):
        return R.from_bits(self.g.debug_buffer(name).view(np.uint16)).reshape(-1, width)

    def chain_logits(self, obs):
        spec = dict((name, self.ref.t(name)) for name, _ in self.ref.specs)
        L = len(self.hidden)
        p = dict(W=[[spec["%s_fc%d/w" % (t, l)] for l in range(L)] for t in ("pi", "vf")], b=[[spec["%s_fc%d/b" % (t, l)] for l in range(L)] for t in ("pi", "vf")],
                 Wh=[spec["pi/w"], spec["vf/w"]], bh=[spec["pi/b"], spec["vf/b"]])
        return R.chain_forward(p, obs, R.rne_bf16, self.A)["mu"]


def names(masked):
    sfx = "<wmcat,mask>" if masked else "<wmcat>"
    return "bf16_step_sequence" + sfx, "bf16_train_sequence" + sfx


def batch(mb):
    return mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"]


@gpu
@both
@cases
def test_stages_against_float64_from_the_devices_own_inputs(case, masked, monkeypatch):
    d = Dev(case)
    g, lay, n, A, nvec = d.g, d.lay, d.n, d.A, d.nvec
    widened(monkeypatch, A)
    obs, u, mk = inputs(d.O, nvec, n, masked)
    chain = d.chain_logits(obs)
    for o, e in M.comps(nvec):
        assert not C.tie_rows(*C.perturbed(chain[:, o:e], u[:, o:e], M.cut(mk, o, e))).any(), "the seed leaves no near-tie (row, component) in the float64 reference"
    mir, th = R.from_bits(g.debug_buffer("bf_theta").view(np.uint16)), g.debug_buffer("theta").view(np.float32)
    a, v, nlp = g.step(obs, u, mask=mk)
    lg, v32 = d.logits_values(n)
    # ---- logits: the float64 product of the device's own bf16 H_L and bf16 weights + the fp32 bias
    Rp, K = R.ru(n, 128), lay.Hp[-1]
    z, s = R.affine(d.bf("bf_h_pi_%d" % (lay.L - 1), K)[:Rp], lay.mat(mir, "pi/w"), lay.mat(th, "pi/b")[0])
    R.check_f32("logits", g.debug_buffer("bf_head_pi").view(np.float32).reshape(-1, lay.Ap)[:Rp], z, 2 * K * R.U * s)
    assert lg.max() - lg.min() <= 20.0, "the inputs keep the logit spread within 20"
    # ---- act: actions [n, K], deterministic actions, neglogp, value from the device's own logits; no (row, component) may be left out
    assert M.check_sampled("action", a, lg, u, nvec, mk) == 0
    M.check_nlp("neglogp", nlp, lg, a, nvec, mk)
    np.testing.assert_array_equal(v, v32)
    M.check_det("deterministic action", g.act_deterministic(obs, mask=mk), lg, nvec, mk)
    # ---- train: d logits (as bf16), exact zeros, slot column sums, loss terms
    mb = M.synth_batch_from(obs, a, v, nlp, 3, CR)
    losses = g.train_step(LR, CR, *batch(mb), mask=mk)
    lg2, v2 = d.logits_values(n)
    np.testing.assert_array_equal(lg2, lg); np.testing.assert_array_equal(v2, v32)
    cr = float(np.float32(CR))
    lo = M.loss(lg, v32, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"], cr, cr, 0.0, ENT, g.cfg.vf_coef, nvec, mk)
    emu = M.emu_loss_dlogits_f32(lg, mb["actions"], mb["advs"], mb["old_neglogp"], CR, ENT, nvec, mk)
    q = d.bf("bf_dhead_pi", lay.Ap)[:Rp]
    M.check_dlogits("d logits", q[:n, :A], lo, R.mismatch_share(R.rne_bf16(emu)[lo["ok"]], lo["dl"][lo["ok"]]))
    for part in (q[n:], q[:, A:], q[:n, :A][~lo["ok"]]):
        assert not part.any() and not np.signbit(part).any(), "dead rows, padding columns and forbidden categories are exactly +0"
    slots = g.debug_buffer("slots_pi").view(np.float32).reshape(-1, 2 * lay.Ap + 8)[:Rp // 16]
    assert not slots[:, lay.Ap:2 * lay.Ap].any(), "the aux slot words are zeros"
    np.testing.assert_array_equal(slots[:, A:lay.Ap], 0.0)
    R.check_f32("slot column sums", slots[:, :A].astype(np.float64).sum(0), lo["db"][0], lo["db"][1] + 2 * len(slots) * R.U * np.abs(lo["dl"]).sum(0))
    for k, name in enumerate(("pg_loss", "vf_loss", "entropy", "approxkl", "clipfrac")):
        R.check_f32(name, losses[k], *lo["terms"][k])
    st, tr = names(masked)                           # (step and act_deterministic: two launches of the step sequence)
    assert g.kernel_count(st) == 2 and g.kernel_count(tr) == 1 and not any(g.kernel_count(x) for x in names(not masked) + ("bf16_step_sequence<mcat>", "bf16_train_sequence<mcat,mask>"))
    g.close()


@gpu
@both
def test_one_component_gives_the_wide_categorical_handles_bits(masked):
    import ppo_cpp_amd
    d = Dev("M321", nvec=(321,))
    gc = ppo_cpp_amd.PPOHip(d.O, 321, list(d.hidden), action_dist="categorical", compute_dtype=1, bf16_head=True, bf16_wide_head=True, ent_coef=ENT)
    gc.set_flat(d.ref.theta.astype(np.float32))
    obs, u, mk = inputs(d.O, d.nvec, d.n, masked)
    a, v, nlp = d.g.step(obs, u, mask=mk)
    ac, vc, nc = gc.step(obs, u, mask=mk)
    np.testing.assert_array_equal(a[:, 0], ac); np.testing.assert_array_equal(v, vc); np.testing.assert_array_equal(nlp, nc)
    np.testing.assert_array_equal(d.g.act_deterministic(obs, mask=mk)[:, 0], gc.act_deterministic(obs, mask=mk))
    mb = M.synth_batch_from(obs, a, v, nlp, 3, CR)
    o_, act, *rest = batch(mb)
    np.testing.assert_array_equal(d.g.train_step(LR, CR, o_, act, *rest, mask=mk), gc.train_step(LR, CR, o_, act[:, 0], *rest, mask=mk))
    for which in range(3):
        np.testing.assert_array_equal(d.g.get_flat(which), gc.get_flat(which))
    d.g.close(); gc.close()


@gpu
@cases
def test_ones_mask_and_evaluate_actions_give_the_steps_bits(case):
    d0, d1 = Dev(case), Dev(case)
    obs, u, mk = inputs(d0.O, d0.nvec, d0.n, True)
    ones = np.ones((d0.n, d0.A), np.float32)
    a, v, nlp = d0.g.step(obs, u)
    for x, y in zip((a, v, nlp), d1.g.step(obs, u, mask=ones)):
        np.testing.assert_array_equal(x, y)
    mb = M.synth_batch_from(obs, a, v, nlp, 11, CR)
    np.testing.assert_array_equal(d0.g.train_step(LR, CR, *batch(mb)), d1.g.train_step(LR, CR, *batch(mb), mask=ones))
    for which in range(3):
        np.testing.assert_array_equal(d0.g.get_flat(which), d1.g.get_flat(which))
    # ppo_evaluate_actions of the drawn action: ppo_step's value and neglogp, plain and masked; the probabilities of a forbidden category are exactly +0
    d0.g.set_bf16_queries(True)
    for m in (None, mk):
        a, v, nlp = d0.g.step(obs, u, mask=m)
        ev_v, ev_nlp, ev_ent = d0.g.evaluate_actions(obs, a, mask=m)
        np.testing.assert_array_equal(ev_nlp, nlp); np.testing.assert_array_equal(ev_v, v)
        lg = d0.logits_values(d0.n)[0]
        R.check_f32("entropy", ev_ent, M.entropy(lg, d0.nvec, m), 1e-4 * len(d0.nvec))
        p = d0.g.action_probability(obs, mask=m)
        assert p.shape == (d0.n, d0.A) and np.allclose(p.sum(1), len(d0.nvec), atol=1e-4)
        assert m is None or (not p[m == 0].any() and not np.signbit(p[m == 0]).any())
    d0.g.close(); d1.g.close()


@gpu
def test_up_to_128_logits_the_flag_changes_nothing():
    d0, d1 = Dev("M129", wide=False, nvec=(2, 124, 2)), Dev("M129", wide=True, nvec=(2, 124, 2))
    obs, u, mk = inputs(d0.O, d0.nvec, d0.n, True)
    for d in (d0, d1):
        d.out = d.g.step(obs, u, mask=mk)
        mb = M.synth_batch_from(obs, *d.out, 3, CR)
        d.out += (d.g.train_step(LR, CR, *batch(mb), mask=mk), d.g.get_flat(0))
        assert d.g.kernel_count("bf16_step_sequence<mcat,mask>") == 1 and d.g.kernel_count("bf16_train_sequence<mcat,mask>") == 1 and not any(d.g.kernel_count(x) for x in names(True))
    for x, y in zip(d0.out, d1.out):
        np.testing.assert_array_equal(x, y)
    d0.g.close(); d1.g.close()


def test_create_refusals_flag_and_names():
    """parse_create and ppo_create_multi_ex answer before any HIP call: no GPU needed"""
    import ppo_cpp_amd
    from ppo_cpp_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "#define PPO_ACT_BF16_WIDE_MULTI_HEAD 0x20000" in open(os.path.join(root, "include", "ppo_hip.h")).read() and capi.ACT_BF16_WIDE_MULTI_HEAD == WIDEM
    lib = ppo_cpp_amd.load_library()
    h = ctypes.c_void_p()

    def refused(nvec, flags, ex=False):
        cfg = capi.PPOConfig()
        lib.ppo_config_default(ctypes.byref(cfg), 7, sum(nvec), 1, (ctypes.c_int32 * 1)(40))
        cfg.compute_dtype = 1
        rc = lib.ppo_create_ex(ctypes.byref(cfg), flags, ctypes.byref(h)) if ex else lib.ppo_create_multi_ex(ctypes.byref(cfg), (ctypes.c_int32 * len(nvec))(*nvec), len(nvec), flags, ctypes.byref(h))
        assert rc != 0
        return lib.ppo_last_error(None).decode()
    msg = refused((1000, 25), MULTI | WIDEM)
    assert "PPO_ACT_BF16_WIDE_MULTI_HEAD" in msg and "1024" in msg and "1025" in msg, msg
    assert refused((64, 65), MULTI) == "ppo_create_multi_ex: PPO_ACT_BF16_MULTI_HEAD: the multi-categorical head of the PPO_BF16 path holds at most 128 logits (sum of nvec is 129)"
    assert "unknown action_dist" in refused((129,), 1 | 0x200 | WIDEM, ex=True)
    with pytest.raises(ValueError, match="multi_bf16_wide_head"):
        ppo_cpp_amd.PPOHip(7, 6, [40], action_dist="categorical", multi_bf16_wide_head=True)
    variants = [lib.ppo_kernel_variant_name(i).decode() for i in range(200) if lib.ppo_kernel_variant_name(i)]
    assert all(name in variants and len(name) < 32 for masked in (False, True) for name in names(masked))
