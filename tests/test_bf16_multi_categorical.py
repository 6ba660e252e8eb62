"""The multi-categorical head (and action masks) of the bf16 matrix-core path: a handle created by ppo_create_multi_ex with PPO_ACT_BF16_MULTI_HEAD and compute_dtype
PPO_BF16 (include/ppo_hip.h).  The GEMMs around the head are every PPO_BF16 handle's (tests/test_bf16_stages.py); here the two kernels that hold the head's arithmetic
(bf16_sample_kernel / bf16_loss_kernel<mcat[,mask]>) are fed the DEVICE's own logits -- the head GEMM's partial products ("bf_head_pi") added in range order -- and
compared with float64 under tests/bf16_cat_ref.py's derived bounds, applied per component and summed in component order (tests/bf16_mcat_ref.py: no bound is derived
there or here).  Bitwise properties follow (one component == the categorical bf16 handle, all-ones mask == unmasked, act model == train model, chained == per-layer,
one-launch assembly == two launches, another split of the same width == the same logits), then end-to-end runs against the library's fp32 <mcat> handle.

Inputs of the stage checks: weights MultiCatRef.init_random(9, pi_gain=1.0), observations and uniforms RandomState(7), masks
multi_categorical_ref.random_masks(RandomState(3), n, nvec).  On the reference's own bf16 chain no (row, component) of any case, masked or plain, has its two best
perturbed logits closer than 1e-4 (test_reference_chain_has_no_near_tie), so the reference leaves out none; the GPU tests print how many they left out.

OBSERVED on an MI355X: see OBSERVED below.
"""
import numpy as np
import pytest

from tests import bf16_cat_ref as C
from tests import bf16_mcat_ref as MC
from tests import bf16_ref as R
from tests.multi_categorical_ref import MultiCatRef, random_masks

gpu = pytest.mark.gpu

CR = 0.16102319955825806
LR = 0.000393141177482903
GAMMA, LAM = 0.99, 0.95
BF16 = 1
ENT = 0.01            # as in tests/test_bf16_categorical.py: large enough for a dropped entropy term to leave the bracket of a bf16 d logit

# (hidden, O, nvec, n): the smallest shapes that reach each way the two kernels can go wrong
CASES = {
    "K2_A8_ragged_dead_rows": ((256, 128), 18, (3, 5), 130),        # A < 16; a ragged last 128-row tile; dead rows in a loss block
    "K2_straddle_lane63": ((1280,), 18, (60, 10), 128),             # a component across the lane-63 / second-element boundary; padding past A = 70
    "K16_A128_full": ((128,), 7, (8,) * 16, 64),                    # K = PPO_MAX_COMPONENTS; A == Ap; every element live
    "K3_uneven_A128": ((128,), 7, (2, 62, 64), 64),                 # a 2-wide component beside one that starts mid-wave and one that is exactly the second elements
    "K2_minimum": ((128,), 7, (2, 2), 64),                          # the smallest head
    "K3_chain": ((512, 512), 64, (6, 6, 6), 2048),                  # chained launches, stage4 staging, many loss blocks
}

# twice the largest mismatch share of rne(fp32 emulation of d logits) against rne(float64) over the six CASES, masked and plain, on the reference's own bf16 chain
# (test_cpu_emulation_share_stays_under_the_recorded_figure prints each: 0 at eight of the twelve, 1.1e-4 at K2_straddle_lane63 plain, 2.44e-4 = 2 of 8192 at
# K16_A128_full and K3_uneven_A128 plain).  The GPU tests cap the DEVICE's own share q != rne(y) at this figure (check_train), and apply rule (2) of
# tests/bf16_ref.py with the emulation's share on the device's own logits beside it, as the categorical module does
CPU_SHARE_MEASURED = 2.45e-4
CPU_SHARES = {"dlogits": 2 * CPU_SHARE_MEASURED}

OBSERVED = """
    stage / output                 units of E     share q != rne(y) (its cap in that case)
    d logits (bf_dhead_pi)         0.13           3.4e-4 at K2_straddle_lane63 plain; 2.4e-4 at K16_A128_full plain and K3_uneven_A128 masked; 0 of 1040 / 637 at K2_A8, 0 of 256 / 193 at
                                                  K2_minimum, 1.4e-4 / 0 at K3_chain plain / masked (cap in every case: CPU_SHARES["dlogits"] = 4.9e-4)
    neglogp (act)                  0.34           (K3_uneven_A128 plain; the row total against the sum of its components' bounds)
    value                          0              (the range-order sum itself)
    pi/b gradient (slot sums)      0.070
    pg_loss / vf_loss / entropy / approxkl / clipfrac   0.0094 / 0.0057 / 0.013 / 0.019 / 0.0033
    (row, component) pairs left out as fp32 near-ties of the perturbed logits: 0 in every case, explicit uniforms and seeded draws (allowed: (n K) // 256)
    update against the fp32 <mcat> handle: entropy rows differ by 2.41e-4 (allowance 2.45e-4 = 10 x the reference's own 2.45e-5) at 64 x 8 / 4 and by 9.0e-5
    (allowance 4.7e-4) at 100 x 10 / 5; host layer: reward curve first-15 0.201, last-15 0.407
"""


def make_ref(hidden, O, nvec, ent_coef=ENT, seed=9, pi_gain=1.0):
    ref = MultiCatRef(O, nvec, hidden, ent_coef=ent_coef)
    ref.init_random(seed, pi_gain)
    return ref


def inputs(O, nvec, n):
    A = int(sum(nvec))
    rng = np.random.RandomState(7)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    return obs, u, random_masks(np.random.RandomState(3), n, nvec)


def chain_params(ref):
    spec = dict((name, ref.t(name)) for name, _ in ref.specs)
    L = len(ref.hidden)
    return dict(W=[[spec["%s_fc%d/w" % (t, l)] for l in range(L)] for t in ("pi", "vf")], b=[[spec["%s_fc%d/b" % (t, l)] for l in range(L)] for t in ("pi", "vf")],
                Wh=[spec["pi/w"], spec["vf/w"]], bh=[spec["pi/b"], spec["vf/b"]])


_CPU_CASES = {}


def cpu_case(case, masked):
    """the reference's own bf16 chain of a case (computed once per case and shared, never changed): logits and values as fp32, a minibatch around the chain's outputs"""
    key = (case, masked)
    if key not in _CPU_CASES:
        hidden, O, nvec, n = CASES[case]
        if (case, "chain") not in _CPU_CASES:
            ref = make_ref(hidden, O, nvec)
            obs, u, mask = inputs(O, nvec, n)
            f = R.chain_forward(chain_params(ref), obs, R.rne_bf16, ref.A)
            _CPU_CASES[(case, "chain")] = (ref, obs, u, mask, f["mu"].astype(np.float32), f["v"].astype(np.float32))
        ref, obs, u, mask, lg, v = _CPU_CASES[(case, "chain")]
        mk = mask if masked else None
        a = MC.sample(lg, u, nvec, mk)
        nlp = MC.nlp_rows(lg, a, nvec, mk)[0]
        mb = MC.synth_batch_from(obs, a.astype(np.float32), v, nlp.astype(np.float32), 3, CR)
        _CPU_CASES[key] = (ref, obs, u, mk, lg, v, mb)
    return _CPU_CASES[key]


# =====================================================================================================================================================
# CPU: the reference and its comparison rules
# =====================================================================================================================================================
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("hidden,O,nvec,n", [((24, 16), 11, (3, 5), 40), ((40,), 7, (60, 10), 24), ((16,), 5, (2, 3, 2, 4), 24)])
def test_reference_agrees_with_the_multi_categorical_reference(hidden, O, nvec, n, masked):
    """tests/bf16_mcat_ref.py, fed EXACT logits, against MultiCatRef (step, and loss_grad by torch autograd) at 1e-9: actions, neglogp, the five loss terms, and the
    d logits -- as the pi/b gradient (their column sums), the pi/w gradient (h^T d logits) and, row by row, the pi/b gradient of one-row minibatches"""
    ref = make_ref(hidden, O, nvec)
    obs, u, mask = inputs(O, nvec, n)
    mk = mask if masked else None
    logits, v = ref.forward(obs)
    ra, rv, rnlp, pert = ref.step(obs, u, mk)
    np.testing.assert_array_equal(MC.sample(logits, u, nvec, mk), ra)
    np.testing.assert_array_equal(MC.deterministic(logits, nvec, mk), ref.act_deterministic(obs, mk))
    np.testing.assert_allclose(MC.nlp_rows(logits, ra, nvec, mk)[0], rnlp, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(MC.entropy(logits, nvec, mk), ref.entropy_of(logits, mk), rtol=1e-9, atol=1e-9)
    mb = MC.synth_batch_from(obs, ra.astype(np.float32), v.astype(np.float32), rnlp.astype(np.float32), 3, CR)
    args = (mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
    ref_losses, ref_grad = ref.loss_grad(*args, CR, mk)
    lo = MC.loss(logits, v, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"], CR, CR, 0.0, ref.ent, ref.vfc, nvec, mk, exact_consts=True)
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
        m1 = None if mk is None else mk[i:i + 1]
        _, g1 = ref.loss_grad(*one, CR, m1)
        lo1 = MC.loss(logits[i:i + 1], v[i:i + 1], one[1], one[2], one[3], one[5], one[4], CR, CR, 0.0, ref.ent, ref.vfc, nvec, m1, exact_consts=True)
        np.testing.assert_allclose(lo1["dl"][0], ref.t("pi/b", g1), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_cpu_emulation_share_stays_under_the_recorded_figure(case, masked):
    """rule (2) takes its cap from NumPy fp32 arithmetic on the same logits: what that emulation shows on the reference's own chain is recorded (CPU_SHARES is twice
    the largest figure printed here)"""
    ref, obs, u, mk, lg, v, mb = cpu_case(case, masked)
    nvec = CASES[case][2]
    cr = float(np.float32(CR))
    lo = MC.loss(lg, v, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"], cr, cr, 0.0, ref.ent, ref.vfc, nvec, mk)
    emu = MC.emu_loss_dlogits_f32(lg, mb["actions"], mb["advs"], mb["old_neglogp"], CR, ref.ent, nvec, mk)
    ok = lo["ok"]
    share = R.mismatch_share(R.rne_bf16(emu)[ok], lo["dl"][ok])
    print(case, "masked" if masked else "plain", "share %.3g of %d" % (share, ok.sum()))
    assert share <= CPU_SHARE_MEASURED, share
    MC.check_dlogits("the emulation itself", R.rne_bf16(emu), lo, share)


@pytest.mark.parametrize("case", list(CASES))
def test_reference_chain_has_no_near_tie(case):
    """no (row, component), masked or plain, whose two best perturbed logits are closer than 1e-4 on the reference's own bf16 chain: check_sampled leaves out none"""
    nvec = CASES[case][2]
    for masked in (False, True):
        ref, obs, u, mk, lg, v, mb = cpu_case(case, masked)
        gap = MC.smallest_gap(lg, u, nvec, mk)
        print(case, "masked" if masked else "plain", "smallest perturbed gap %.3g" % gap)
        assert gap >= 1e-4, gap
        assert MC.check_sampled("the reference itself", MC.sample(lg, u, nvec, mk).astype(np.float32), lg, u, nvec, mk) == 0
        MC.check_det("the reference itself", MC.deterministic(lg, nvec, mk).astype(np.float32), lg, nvec, mk)


def test_comparison_rules_reject_planted_faults():
    """on the reference's own data (nothing runs on a GPU): the stand-in for a kernel's output is perturbed the way a wrong walk over the components would be, and the
    functions the GPU tests call must reject it
      1. a component's entropy dropped from the gradient              2. H of the neighbouring component used
      3. an action index taken as global instead of within-component  4. the argmax of one component leaking one column into the next
      5. a forbidden column with a non-zero d logit"""
    case = "K2_A8_ragged_dead_rows"
    ref, obs, u, mk, lg, v, mb = cpu_case(case, True)
    nvec = CASES[case][2]
    off = MC.offsets(nvec)
    n, A = lg.shape
    cr = float(np.float32(CR))
    lo = MC.loss(lg, v, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"], cr, cr, 0.0, ref.ent, ref.vfc, nvec, mk)
    emu = MC.emu_loss_dlogits_f32(lg, mb["actions"], mb["advs"], mb["old_neglogp"], CR, ref.ent, nvec, mk)
    share = R.mismatch_share(R.rne_bf16(emu)[lo["ok"]], lo["dl"][lo["ok"]])
    good = R.rne_bf16(emu)
    MC.check_dlogits("the stand-in itself", good, lo, share)
    R.check_f32("the stand-in's pi/b sums", emu.sum(0, dtype=np.float32), *lo["db"])
    # 1.
    dropped = MC.emu_loss_dlogits_f32(lg, mb["actions"], mb["advs"], mb["old_neglogp"], CR, ref.ent, nvec, mk, drop_entropy_of=1)
    np.testing.assert_array_equal(dropped[:, :off[1]], emu[:, :off[1]])
    with pytest.raises(AssertionError, match="not rne|leave the bracket"):
        MC.check_dlogits("d logits without component 1's entropy term", R.rne_bf16(dropped), lo, share)
    with pytest.raises(AssertionError, match="further from the float64 value"):
        R.check_f32("pi/b sums without component 1's entropy term", dropped.sum(0, dtype=np.float32), *lo["db"])
    # 2.  d logits_j carries ent_coef g p_j H_k: with the neighbour's H the element moves by ent_coef g p_j (H_other - H_k)
    g32 = np.float32(1.0) / np.float32(n)
    hds = MC.head(lg, nvec, mk)
    swapped = emu.copy()
    for k, other in ((0, 1), (1, 0)):
        shift = (np.float32(ref.ent) * g32) * (hds[k]["p"] * (lo["H_k"][other] - lo["H_k"][k])[:, None])
        swapped[:, off[k]:off[k + 1]] += np.where(hds[k]["ok"], shift, 0.0).astype(np.float32)
    with pytest.raises(AssertionError, match="not rne|leave the bracket"):
        MC.check_dlogits("H of the neighbouring component", R.rne_bf16(swapped), lo, share)
    with pytest.raises(AssertionError, match="further from the float64 value"):
        R.check_f32("pi/b sums with H of the neighbouring component", swapped.sum(0, dtype=np.float32), *lo["db"])
    # 3.
    smp = MC.sample(lg, u, nvec, mk).astype(np.float32)
    det = MC.deterministic(lg, nvec, mk).astype(np.float32)
    MC.check_sampled("the stand-in itself", smp, lg, u, nvec, mk); MC.check_det("the stand-in itself", det, lg, nvec, mk)
    with pytest.raises(AssertionError, match="not category indices"):
        MC.check_sampled("global indices", smp + off[:-1].astype(np.float32), lg, u, nvec, mk)
    with pytest.raises(AssertionError, match="not category indices"):
        MC.check_det("global indices", det + off[:-1].astype(np.float32), lg, nvec, mk)
    nlp_good = MC.nlp_rows(lg, smp, nvec, mk)[0].astype(np.float32)
    MC.check_nlp("the stand-in itself", nlp_good, lg, smp, nvec, mk)
    # (the loss side: component 1's neglogp read at component 0's index)
    a = mb["actions"].astype(np.int64)
    wrong_nlp = (MC.nlp_rows(lg, np.stack([a[:, 0], a[:, 0] % nvec[1]], 1), nvec, None)[0]).astype(np.float32)
    assert (a[:, 1] != a[:, 0] % nvec[1]).any()
    with pytest.raises(AssertionError, match="further from the float64 value"):
        MC.check_nlp("component 1's action read from column 0", wrong_nlp, lg, a, nvec, None)
    # 4.  unmasked logits: component 0's argmax taken over its columns AND the first column of component 1
    ext = np.argmax(lg[:, :off[1] + 1].astype(np.float64), axis=1)
    leak_rows = np.nonzero(ext == off[1])[0]
    assert leak_rows.size, "the case has rows whose logit at component 1's first column beats all of component 0's"
    det0 = MC.deterministic(lg, nvec, None).astype(np.float32)
    MC.check_det("the stand-in itself", det0, lg, nvec, None)
    for clamp in (False, True):                                       # as it leaks (index n_0), and brought back inside by min(i, e - 1)
        bad = det0.copy()
        rows_ = leak_rows if not clamp else leak_rows[det0[leak_rows, 0] != nvec[0] - 1]
        assert rows_.size
        bad[rows_, 0] = nvec[0] - 1 if clamp else nvec[0]
        with pytest.raises(AssertionError, match="not category indices|lowest-index argmax"):
            MC.check_det("component 0's argmax over one column too many", bad, lg, nvec, None)
    # 5.
    bad = good.copy()
    i, j = np.argwhere(~lo["ok"])[0]
    bad[i, j] = np.float32(2.0 ** -20)
    with pytest.raises(AssertionError, match="forbidden"):
        MC.check_dlogits("a forbidden column with a gradient", bad, lo, share)


NEW_NAMES = ("bf16_step_sequence<mcat>", "bf16_step_sequence<mcat,mask>", "bf16_train_sequence<mcat>", "bf16_train_sequence<mcat,mask>")


def test_flag_is_declared_with_its_value_and_the_names_fit():
    import os
    from ppo_cpp_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "ppo_hip.h")).read()
    assert "#define PPO_ACT_BF16_MULTI_HEAD 0x1000" in src and "#define PPO_ACT_BF16_HEAD 0x200" in src and "#define PPO_ABI_VERSION 3" in src
    assert capi.ACT_BF16_MULTI_HEAD == 0x1000 and capi.ACT_BF16_HEAD == 0x200
    hip = open(os.path.join(root, "ppo_cpp_amd", "csrc", "ppo_hip.hip")).read()
    for name in NEW_NAMES:
        assert len(name) < 32 and '"%s"' % name in hip          # ppo_kernel_counts' char[32]


def create_multi_ex(nvec, flags, **overrides):
    """ppo_create_multi_ex through ctypes; returns (status, message)"""
    import ctypes
    import ppo_cpp_amd
    from ppo_cpp_amd.capi import PPOConfig
    lib = ppo_cpp_amd.load_library()
    cfg = PPOConfig()
    hid = (ctypes.c_int32 * 2)(64, 64)
    lib.ppo_config_default(ctypes.byref(cfg), 18, sum(nvec), 2, hid)
    for k, v in overrides.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    nv = (ctypes.c_int32 * 32)(*nvec)
    rc = lib.ppo_create_multi_ex(ctypes.byref(cfg), nv, len(nvec), flags, ctypes.byref(h))
    msg = lib.ppo_last_error(None).decode() if rc != 0 else ""
    if rc == 0:
        lib.ppo_destroy(h)
    return rc, msg


def test_the_flag_is_a_known_bit_of_ppo_create_multi_ex():
    """(the flags are checked before a device is looked for: without a GPU a known bit gets as far as "no HIP device", an unknown one is named)"""
    import torch
    rc, msg = create_multi_ex([3, 5], 0x1000)
    assert "unknown flag" not in msg, msg
    if not torch.cuda.is_available():
        assert rc != 0 and "no HIP device" in msg, msg
    rc, msg = create_multi_ex([3, 5], 0x800)
    assert rc != 0 and "unknown flag bit 0x800" in msg, msg
    rc, msg = create_multi_ex([3, 5], 0, compute_dtype=1)
    assert rc != 0 and "the multi-categorical head runs on the PPO_F32 path" in msg, msg
    rc, msg = create_multi_ex([3, 5], 0x200, compute_dtype=1)
    assert rc != 0 and "the multi-categorical head runs on the PPO_F32 path" in msg, msg
    rc, msg = create_multi_ex([65, 64], 0x1000, compute_dtype=1)
    assert rc != 0 and "128" in msg and "129" in msg, msg


# =====================================================================================================================================================
# GPU
# =====================================================================================================================================================
class Dev:
    """a multi-categorical PPO_BF16 handle with the reference's weights and typed reads of its workspaces"""

    def __init__(self, hidden, O, nvec, ent_coef=ENT, seed=9, pi_gain=1.0, masking=False, **kw):
        import ppo_cpp_amd
        self.ref = make_ref(hidden, O, nvec, ent_coef, seed, pi_gain)
        self.g = ppo_cpp_amd.PPOHip(O, None, list(hidden), action_dist="multi_categorical", nvec=list(nvec), compute_dtype=BF16, bf16_head=True, ent_coef=ent_coef, **kw)
        assert list(self.g.tensors) == [(n, s) for n, s in self.ref.specs], "4L + 4 tensors, no pi/logstd"
        assert self.g.nvec == list(nvec) and self.g.action_width == len(nvec)
        self.g.set_flat(self.ref.theta.astype(np.float32))
        if masking:
            self.g.set_action_masking(True)
        self.O, self.A, self.nvec, self.K = O, int(sum(nvec)), tuple(nvec), len(nvec)
        self.lay = R.Layout(O, self.A, hidden)                 # (the padded vector keeps the logstd slot: the Gaussian layout's offsets hold)
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
    print("\n[bf16 multi-categorical] %s" % what)
    for k, v in sorted(d.rec.items()):
        print("    %-34s %s" % (k, "  ".join("%s=%.3g" % kv for kv in sorted(v.items()))))


def allowed_at(mk, acts, nvec):
    """[n, K] bool: the mask entry of every component's action"""
    off = MC.offsets(nvec)
    a = np.asarray(acts).astype(np.int64)
    return np.stack([mk[np.arange(a.shape[0]), off[k] + a[:, k]] != 0 for k in range(len(nvec))], axis=1)


def check_act(d, obs, u, mk, tag):
    g, n, nvec = d.g, obs.shape[0], d.nvec
    a, v, nlp = g.step(obs, u, mask=mk)
    lg, v32 = d.logits_values(n)
    MC.check_sampled(tag + " action", a, lg, u, nvec, mk)
    MC.check_nlp(tag + " neglogp", nlp, lg, a, nvec, mk, d.rec)
    R.check_f32(tag + " value", v, v32, 0.0, rec=d.rec)           # (the value IS the range-order sum: bound 0)
    det = g.act_deterministic(obs, mask=mk)
    MC.check_det(tag + " deterministic action", det, d.logits_values(n)[0], nvec, mk)
    np.testing.assert_array_equal(d.logits_values(n)[0], lg, err_msg="the deterministic pass leaves the same logits")
    if mk is not None:
        assert allowed_at(mk, a, nvec).all() and allowed_at(mk, det, nvec).all()
        g.seed(3)
        assert allowed_at(mk, g.step(obs, mask=mk)[0], nvec).all()  # the counter draw under the mask
    return a, v, nlp


def check_train(d, obs, a, v, nlp, mk, tag, seed=3, floor=0.0, normal=0.0):
    """floor, normal: bf16_cat_ref.check_dlogits' underflow floor (added to every bound here, once per summed row for the pi/b sums) and the size from which a d logit
    counts in the rounding share; 0 and 0 for logits of order 1"""
    g, lay, rec, nvec = d.g, d.lay, d.rec, d.nvec
    n, A = obs.shape[0], d.A
    Rp = R.ru(n, 128)
    mb = MC.synth_batch_from(obs, a, v, nlp, seed, CR)
    losses = g.train_step(LR, CR, mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"], mask=mk)
    lg, v32 = d.logits_values(n)
    cr = float(np.float32(CR))
    lo = MC.loss(lg, v32, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"], cr, cr, 0.0, g.cfg.ent_coef, g.cfg.vf_coef, nvec, mk)
    emu = MC.emu_loss_dlogits_f32(lg, mb["actions"], mb["advs"], mb["old_neglogp"], CR, g.cfg.ent_coef, nvec, mk)
    q = d.bf("bf_dhead_pi", lay.Ap)[:Rp]
    sel = MC.C.normal_size(lo, normal)
    emu_share = R.mismatch_share(R.rne_bf16(emu)[sel], lo["dl"][sel]) if sel.any() else 0.0
    share = R.mismatch_share(q[:n, :A][sel], lo["dl"][sel]) if sel.any() else 0.0
    print("%s d logits: emulation share on the device's logits %.3g, device share %.3g of %d" % (tag, emu_share, share, sel.sum()))
    edge = bool(floor or normal)        # (CPU_SHARES is what the emulation showed on THIS file's six CASES; other inputs take the emulation's share on their own logits, rule (2) as it stands)
    MC.check_dlogits(tag + " d logits", q[:n, :A], lo, emu_share if edge else min(emu_share, CPU_SHARES["dlogits"]), rec, floor, normal)
    assert edge or share <= CPU_SHARES["dlogits"], "%s: %.4g of the d logits are not rne(y) (cap %.4g = twice the CPU emulation's largest share)" % (tag, share, CPU_SHARES["dlogits"])
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


def only_new_names(kc, step=None, train=None):
    """among the bf16_*sequence* names only the four new ones are counted; step / train: the suffix that must be"""
    for name, c in kc.items():
        if name.startswith("bf16_step_sequence") or name.startswith("bf16_train_sequence"):
            assert c == 0 or name in NEW_NAMES, kc
    for which, sfx in (("bf16_step_sequence", step), ("bf16_train_sequence", train)):
        if sfx is not None:
            other = "<mcat>" if sfx == "<mcat,mask>" else "<mcat,mask>"
            assert kc[which + sfx] > 0 and kc[which + other] == 0, kc
    for name in ("policy_step_kernel<mcat>", "policy_step_kernel<mcat,mask>", "train_fwd_bwd_kernel<mcat>", "train_fwd_bwd_kernel<mcat,mask>"):
        assert kc[name] == 0, kc


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("case", list(CASES))
def test_head_stages_from_the_devices_own_logits(case, masked):
    """ppo_step, ppo_act_deterministic and ppo_train_step at the six shapes, masked and plain: actions and deterministic actions [n, K], neglogp, value from the
    device's own logits; d logits (bracket, exact-rounding share, exact +0), the pi/b gradient, the five loss terms and the aux slot words from the train pass's logits"""
    hidden, O, nvec, n = CASES[case]
    d = Dev(hidden, O, nvec)
    obs, u, mask = inputs(O, nvec, n)
    mk = mask if masked else None
    a, v, nlp = check_act(d, obs, u, mk, "act")
    assert a.shape == (n, len(nvec))
    check_train(d, obs, a, v, nlp, mk, "train")
    kc = d.g.kernel_counts()
    sfx = "<mcat,mask>" if masked else "<mcat>"
    only_new_names(kc, sfx, sfx)
    assert kc["bf16_step_sequence" + sfx] >= 2 and kc["bf16_train_sequence" + sfx] == 1, kc
    report(d, "%s %s %s" % (case, CASES[case], "masked" if masked else "plain"))
    d.close()


def upload(g, fields):
    for f, x in fields.items():
        g.rollout_set(f, np.asarray(x, np.float32))


def ref_fields(ref, rng, E, T, masks=None):
    """an uploaded rollout built by the reference: the actions [T, E, K] are consistent with the masks"""
    O, A, K = ref.O, ref.A, ref.K
    obs = rng.uniform(-1, 1, (T, E, O)).astype(np.float32)
    a, v, nlp, _ = ref.step(obs.reshape(-1, O), rng.uniform(size=(T * E, A)), None if masks is None else masks.reshape(T * E, A))
    f = {"obs": obs, "actions": a.reshape(T, E, K), "values": v.reshape(T, E), "neglogp": nlp.reshape(T, E) + rng.normal(scale=0.1, size=(T, E)),
         "dones": (rng.uniform(size=(T, E)) < 0.02).astype(np.float32), "rewards": rng.normal(size=(T, E)),
         "returns": v.reshape(T, E) + rng.normal(scale=0.5, size=(T, E))}
    if masks is not None:
        f["masks"] = masks
    return f


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("A", [6, 70, 128])
def test_one_component_gives_the_categorical_bf16_handles_bits(A, masked):
    """nvec = [A] against PPO_ACT_CATEGORICAL | PPO_ACT_BF16_HEAD with act_dim = A: every output of step, act_deterministic and train_step, the gradient, and the
    weights and Adam slots after an update"""
    import ppo_cpp_amd
    from tests.masked_categorical_ref import random_masks as cat_masks
    hidden, O, n = (256, 128), 18, 130
    E, T, nmb, epochs = 16, 8, 1, 2
    d = Dev(hidden, O, (A,), masking=masked)
    gc = ppo_cpp_amd.PPOHip(O, A, list(hidden), action_dist="categorical", compute_dtype=BF16, bf16_head=True, ent_coef=ENT)
    gc.set_flat(d.ref.theta.astype(np.float32))
    if masked:
        gc.set_action_masking(True)
    gm = d.g
    obs, u, _ = inputs(O, (A,), n)
    mk = cat_masks(np.random.RandomState(3), n, A) if masked else None
    am, vm, nm = gm.step(obs, u, mask=mk)
    ac, vc, nc = gc.step(obs, u, mask=mk)
    assert am.shape == (n, 1)
    np.testing.assert_array_equal(am[:, 0], ac); np.testing.assert_array_equal(vm, vc); np.testing.assert_array_equal(nm, nc)
    np.testing.assert_array_equal(gm.act_deterministic(obs, mask=mk)[:, 0], gc.act_deterministic(obs, mask=mk))
    gm.seed(5); gc.seed(5)
    np.testing.assert_array_equal(gm.step(obs, mask=mk)[0][:, 0], gc.step(obs, mask=mk)[0])
    for it in range(2):
        mb = C.synth_batch_from(obs, ac, vc, nc, 11 + it, CR)
        args = (mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
        np.testing.assert_array_equal(gm.train_step(LR, CR, mb["obs"], mb["actions"].reshape(n, 1), *args, mask=mk), gc.train_step(LR, CR, mb["obs"], mb["actions"], *args, mask=mk))
        for x, y in zip(gm.last_grad(), gc.last_grad()):
            np.testing.assert_array_equal(x, y)
        for which in range(3):
            np.testing.assert_array_equal(gm.get_flat(which), gc.get_flat(which))
    rng = np.random.RandomState(5)
    masks = cat_masks(rng, T * E, A, special=False).reshape(T, E, A) if masked else None
    fields = ref_fields(d.ref, rng, E, T, masks)
    perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
    out = []
    for g in (gm, gc):
        g.norm_init(E, GAMMA); g.rollout_alloc(E, T)
        upload(g, dict(fields, actions=fields["actions"] if g is gm else fields["actions"][..., 0]))
        out.append(g.update(LR, CR, epochs, nmb, perms))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    for which in range(3):
        np.testing.assert_array_equal(gm.get_flat(which), gc.get_flat(which))
    only_new_names(gm.kernel_counts(), "<mcat,mask>" if masked else "<mcat>", "<mcat,mask>" if masked else "<mcat>")
    d.close(); gc.close()


@gpu
@pytest.mark.parametrize("O,nvec", [(18, (3, 5, 2, 8)), (64, (6, 6, 6, 6))], ids=["O18", "O64_K4"])
def test_all_ones_masks_give_the_unmasked_bits(O, nvec):
    """(O = 64, K = 4: observation and action rows are whole 16-byte quads, so the unmasked handle's update takes the 16-byte epoch gather with the bf16 staging fused
    into it where the masking handle takes the element-wise gather and the separate staging launch: the same bits through both)"""
    hidden, n = (256, 128), 130
    E, T, nmb, epochs = 32, 8, 2, 2
    A = sum(nvec)
    d0, d1 = Dev(hidden, O, nvec), Dev(hidden, O, nvec, masking=True)
    g0, g1 = d0.g, d1.g
    obs, u, _ = inputs(O, nvec, n)
    ones = np.ones((n, A), np.float32)
    for x, y in zip(g0.step(obs, u), g1.step(obs, u, mask=ones)):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(g0.act_deterministic(obs), g1.act_deterministic(obs, mask=ones))
    for it in range(2):
        a, v, nlp = g0.step(obs, u)
        mb = MC.synth_batch_from(obs, a, v, nlp, 11 + it, CR)
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
    only_new_names(g0.kernel_counts(), "<mcat>", "<mcat>")
    only_new_names(g1.kernel_counts(), "<mcat,mask>", "<mcat,mask>")
    d0.close(); d1.close()


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("case", ["K2_A8_ragged_dead_rows", "K2_straddle_lane63", "K16_A128_full"])
def test_act_model_and_train_model_give_the_same_neglogp_bits(case, masked):
    """old_neglogp = step(..)[2] on the same rows, actions and weights: the first train step's ratio is exactly 1 (approxkl == 0.0, clipfrac == 0.0) -- the sample
    and the loss kernel share their reduction shape per component (cat_row_norm / cat_row_pick) and add the components alike"""
    hidden, O, nvec, n = CASES[case]
    d = Dev(hidden, O, nvec)
    obs, u, mask = inputs(O, nvec, n)
    mk = mask if masked else None
    a, v, nlp = d.g.step(obs, u, mask=mk)
    rng = np.random.RandomState(1)
    adv = rng.normal(size=n).astype(np.float32)
    losses = d.g.train_step(LR, CR, obs, a, adv, (v + rng.normal(scale=0.5, size=n)).astype(np.float32), nlp, v, mask=mk)
    assert losses[3] == 0.0 and losses[4] == 0.0, losses
    assert np.isfinite(losses).all() and losses[2] > 0
    d.close()


def run_steps(d, obs, u, mk, steps=2):
    out = []
    for it in range(steps):
        a, v, nlp = d.g.step(obs, u, mask=mk)
        mb = MC.synth_batch_from(obs, a, v, nlp, 40 + it, CR)
        losses = d.g.train_step(LR, CR, mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"], mask=mk)
        out += [a, v, nlp, losses, d.g.last_grad()[0]] + [d.g.get_flat(w) for w in range(3)]
    return out


@gpu
@pytest.mark.parametrize("switch", ["PPO_HIP_NO_BF16_CHAIN", "PPO_HIP_NO_REDUCE_ADAM"])
def test_launch_forms_agree_bitwise_with_the_multi_categorical_head_in_between(switch, monkeypatch):
    """the chained launch against a launch per layer, and the one-launch assembly + clip + Adam against the two launches, at K3_chain, masked"""
    hidden, O, nvec, n = CASES["K3_chain"]
    obs, u, mask = inputs(O, nvec, n)
    monkeypatch.delenv(switch, raising=False)
    d = Dev(hidden, O, nvec)
    want = run_steps(d, obs, u, mask)
    if switch == "PPO_HIP_NO_BF16_CHAIN":
        d.g.debug_raise_chain_error()                          # (refused by a handle that does not chain: this one did)
    d.close()
    monkeypatch.setenv(switch, "1")
    d = Dev(hidden, O, nvec)
    got = run_steps(d, obs, u, mask)                           # (PPO_HIP_NO_REDUCE_ADAM is read again when a step is enqueued)
    monkeypatch.delenv(switch)
    for x, y in zip(want, got):
        np.testing.assert_array_equal(x, y)
    kc = d.g.kernel_counts()
    assert kc["bf16_train_sequence<mcat,mask>"] == 2 and (kc["bf16_reduce_adam_kernel"] == 0) == (switch == "PPO_HIP_NO_REDUCE_ADAM"), kc
    d.close()


@gpu
def test_another_split_of_the_same_width_takes_the_same_vector_and_gives_the_same_logits():
    hidden, O, n = (256, 128), 18, 130
    da, db = Dev(hidden, O, (3, 5, 2, 8)), Dev(hidden, O, (9, 9), seed=10)
    assert da.g.tensors == db.g.tensors and da.g.P == db.g.P and db.g.nvec == [9, 9] and db.g.action_width == 2
    for which in range(3):
        db.g.set_flat(da.g.get_flat(which), which)
        np.testing.assert_array_equal(db.g.get_flat(which), da.g.get_flat(which))
    obs, u, _ = inputs(O, (9, 9), n)
    aa, va, _ = da.g.step(obs, u); ab, vb, _ = db.g.step(obs, u)
    assert aa.shape == (n, 4) and ab.shape == (n, 2)
    np.testing.assert_array_equal(da.logits_values(n)[0], db.logits_values(n)[0])
    np.testing.assert_array_equal(va, vb)
    MC.check_sampled("the other split", ab, db.logits_values(n)[0], u, (9, 9))
    da.close(); db.close()


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_seeded_draws_are_the_counter_models_uniforms_at_the_global_logit_index(masked):
    """without explicit noise: the actions are those of the reference fed tests/counter_draws_ref's uniforms at (seed, row, step, j), j the GLOBAL logit index"""
    from tests import counter_draws_ref as M
    hidden, O, nvec, n = CASES["K3_uneven_A128"]
    d = Dev(hidden, O, nvec)
    obs, _, mask = inputs(O, nvec, n)
    mk = mask if masked else None
    d.g.seed(1234)
    left = 0
    for step in range(2):
        a, v, nlp = d.g.step(obs, mask=mk)
        lg, _ = d.logits_values(n)
        um = M.counter_uniforms(M.seed_key(1234), np.arange(n), step, d.A).astype(np.float32)
        left += MC.check_sampled("seeded step %d" % step, a, lg, um, nvec, mk)
        MC.check_nlp("seeded step %d neglogp" % step, nlp, lg, a, nvec, mk, d.rec)
    print("seeded draws: (row, component) pairs left out %d" % left)
    d.close()


@gpu
def test_on_device_sampling_follows_the_product_of_the_components_softmaxes():
    """65536 copies of one observation, (128,) / 7 / (3, 4), pi_gain 3: the joint frequencies of the 12 action pairs within 4 sigma of the product of the
    components' softmaxes of the device's own logits of row 0"""
    hidden, O, nvec, n = (128,), 7, (3, 4), 65536
    d = Dev(hidden, O, nvec, pi_gain=3.0)
    obs = np.tile(np.random.RandomState(2).uniform(-1, 1, (1, O)).astype(np.float32), (n, 1))
    d.g.seed(11)
    a, _, nlp = d.g.step(obs)
    lg, _ = d.logits_values(n)
    assert np.all(lg == lg[0])
    p0, p1 = [hd["p"][0] for hd in MC.head(lg[:1], nvec)]
    p = np.outer(p0, p1)
    assert p.max() < 0.9 and p.min() > 1e-4, p
    ai = a.astype(np.int64)
    freq = np.bincount(ai[:, 0] * nvec[1] + ai[:, 1], minlength=12).reshape(3, 4) / n
    sigma = np.sqrt(p * (1 - p) / n)
    assert np.all(np.abs(freq - p) <= 4 * sigma), (freq, p, sigma)
    d.g.seed(11)
    np.testing.assert_array_equal(d.g.step(obs)[0], a)
    d.g.seed(12)
    assert np.any(d.g.step(obs)[0] != a)
    d.close()


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("case", ["K2_A8_ragged_dead_rows", "K2_straddle_lane63"])
def test_gradient_of_one_train_step_against_the_float64_reference(case, masked):
    """against MultiCatRef.loss_grad (torch float64 autograd on the fp32 weights): cosine > 0.995 per tensor that carries more than 1e-3 of the norm, global norm within
    3 % (the criteria of tests/test_bf16_categorical.py)"""
    hidden, O, nvec, n = CASES[case]
    d = Dev(hidden, O, nvec)
    obs, u, mask = inputs(O, nvec, n)
    mk = mask if masked else None
    a, v, nlp, _ = d.ref.step(obs, u, mk)
    mb = MC.synth_batch_from(obs, a.astype(np.float32), v.astype(np.float32), nlp.astype(np.float32), 3, CR)
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


def reference_entropy_deviation(ref, obs_rows, masks_rows, idx_per_mb):
    """what bf16 operands do to a minibatch's mean entropy IN THE REFERENCE: the fp32 weights' logits against bf16_ref.chain_forward(.., rne_bf16, ..) logits through the
    same per-component head; the largest |difference| over the given minibatches"""
    exact = MC.entropy(ref.forward(obs_rows)[0], ref.nvec, masks_rows)
    rounded = MC.entropy(R.chain_forward(chain_params(ref), obs_rows, R.rne_bf16, ref.A)["mu"], ref.nvec, masks_rows)
    return max(abs(exact[i].mean() - rounded[i].mean()) for i in idx_per_mb), float(np.abs(exact - rounded).mean())


@gpu
@pytest.mark.parametrize("E,T,nmb", [(64, 8, 4), (100, 10, 5)])
def test_update_tracks_the_fp32_multi_categorical_handle(E, T, nmb):
    """the same uploaded rollout (built by the reference under masks), the same explicit permutations, two epochs at (256, 128) / 18 / (3, 5, 2, 8): the bf16 handle
    against the library's fp32 <mcat> handle under tests/test_bf16_categorical.py's tolerances.  The entropy allowance is RATE_FACTOR (10) x the deviation the REFERENCE
    shows between fp32 and rne_bf16-chain logits on the first epoch's minibatches, computed on the CPU and printed."""
    import ppo_cpp_amd
    hidden, O, nvec, epochs = (256, 128), 18, (3, 5, 2, 8), 2
    A = sum(nvec)
    db = Dev(hidden, O, nvec, masking=True)
    gf = ppo_cpp_amd.PPOHip(O, None, list(hidden), action_dist="multi_categorical", nvec=list(nvec), ent_coef=ENT)
    gf.set_flat(db.ref.theta.astype(np.float32)); gf.set_action_masking(True)
    rng = np.random.RandomState(9)
    masks = random_masks(rng, T * E, nvec, special=False).reshape(T, E, A)
    fields = ref_fields(db.ref, rng, E, T, masks)
    perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
    rows = {}
    for name, g in (("f32", gf), ("bf16", db.g)):
        g.norm_init(E, GAMMA); g.rollout_alloc(E, T)
        upload(g, fields)
        rows[name] = g.update(LR, CR, epochs, nmb, perms)[0]
    rb, rf = rows["bf16"], rows["f32"]
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
    only_new_names(db.g.kernel_counts(), None, "<mcat,mask>")
    kf = gf.kernel_counts()
    assert kf["train_fwd_bwd_kernel<mcat,mask>"] > 0 and all(kf[name] == 0 for name in NEW_NAMES), kf
    db.close(); gf.close()


@gpu
def test_collect_synthetic_and_the_masked_rollout_entry_points():
    """ppo_collect_synthetic (E = 64, T = 4, seeded on-device uniforms): integer actions [T, E, K] in [0, n_k), every stored neglogp is the reference neglogp of the
    stored action from the logits a fresh pass leaves for the stored observation; one seed twice agrees bitwise.  Then the rollout entry points under
    ppo_set_action_masking: rollout_act(t, mask=..) returns [E, K] integer actions every component of which its mask allows, field 8 round-trips bitwise"""
    from oracle import oracle as o
    hidden, O, nvec = (256, 128), 18, (3, 5, 2, 8)
    E, T = 64, 4
    A, K = sum(nvec), len(nvec)
    d = Dev(hidden, O, nvec)
    g = d.g
    runs = []
    for seed in (77, 77, 78):
        g.norm_init(E, GAMMA); g.rollout_alloc(E, T)
        g.collect_synthetic(seed, GAMMA, LAM, None)
        runs.append({f: g.rollout_get(f) for f in ("obs", "actions", "values", "neglogp", "returns")})
    for f in runs[0]:
        np.testing.assert_array_equal(runs[0][f], runs[1][f], err_msg=f)
    assert np.mean(runs[0]["actions"] != runs[2]["actions"]) > 0.3
    ro = runs[2]
    acts = ro["actions"].reshape(-1, K)
    assert ro["actions"].shape == (T, E, K) and np.all(acts == np.floor(acts)) and acts.min() >= 0 and np.all(acts.max(0) < np.array(nvec)) and np.all(acts.max(0) > 0)
    obs = ro["obs"].reshape(T * E, O)
    v = g.value(obs)                                           # a fresh pass over the stored observations (they are stored normalised)
    lg, v32 = d.logits_values(T * E)
    MC.check_nlp("collect neglogp", ro["neglogp"].reshape(-1), lg, acts, nvec, None, d.rec)
    np.testing.assert_array_equal(ro["values"].reshape(-1), v32)
    np.testing.assert_array_equal(v, v32)
    only_new_names(g.kernel_counts(), "<mcat>", None)
    d.close()
    # the host-Env entry points with masks
    d = Dev(hidden, O, nvec, masking=True)
    g = d.g
    E = 17
    rng = np.random.RandomState(E + 1)
    masks = np.stack([random_masks(rng, E, nvec) for _ in range(T)])
    g.norm_init(E); g.rollout_alloc(E, T)
    raw, _, _ = o.seeded_env_step(99, 0, E, 0, O)
    g.rollout_reset(raw)
    g.seed(21)
    acts = []
    for t in range(T):
        a = g.rollout_act(t, None if t % 2 else rng.uniform(size=(E, A)).astype(np.float32), mask=masks[t])
        assert a.shape == (E, K) and np.all(a == np.floor(a)) and a.min() >= 0 and np.all(a < np.array(nvec)), a
        assert allowed_at(masks[t], a, nvec).all(), "step %d: an action its component's mask forbids" % t
        acts.append(a)
        raw, rew, dn = o.seeded_env_step(99, 0, E, t + 1, O)
        g.rollout_observe(t, raw, rew, dn)
    g.rollout_finish(GAMMA, LAM)
    np.testing.assert_array_equal(np.array(acts), g.rollout_get("actions"))
    np.testing.assert_array_equal(g.rollout_get("masks"), masks)
    other = np.stack([random_masks(rng, E, nvec, special=False) for _ in range(T)])
    g.rollout_set("masks", other)
    np.testing.assert_array_equal(g.rollout_get("masks"), other)
    assert np.isfinite(g.rollout_get("returns")).all()
    kc = g.kernel_counts()
    only_new_names(kc)
    assert kc["bf16_step_sequence<mcat,mask>"] >= T, kc            # (the value-only pass of rollout_finish takes no mask)
    d.close()


@gpu
def test_ppo2_learns_the_multi_discrete_target_task_on_the_bf16_path():
    """tests/test_multi_discrete.test_ppo2_learns_the_multi_discrete_target_task with compute_dtype=1: ppo_host_learn_multi passes PPO_ACT_BF16_MULTI_HEAD through
    PPO2::create_handle.  That test's RISE / BAND / reference figure (0.123 / 0.089 / 0.419, derived there from the NumPy reference loop): the last-15 mean reward over
    the first-15, and its distance from the reference's.  Measured on an MI355X: first-15 0.201, last-15 0.407."""
    from ppo_cpp_amd import hostapi
    RISE, BAND, REF_LAST15 = 0.123, 0.089, 0.419
    got = hostapi.learn_curve(16, 64, [64, 64], 80, 4, 4, 2e-3, 0.2, seed=11, nvec=(6, 6, 6), compute_dtype=1)
    only_new_names(got["kernel_counts"], "<mcat>", "<mcat>")
    c = got["reward_curve"]
    first, last = c[:15].mean(), c[-15:].mean()
    print("reward curve first-15 %.3f last-15 %.3f" % (first, last))
    assert last - first >= RISE, (first, last)
    assert abs(last - REF_LAST15) <= BAND, (last, REF_LAST15)


@gpu
def test_ppo2_runs_the_masked_multi_discrete_env_on_the_bf16_path_without_a_forbidden_action():
    from ppo_cpp_amd import hostapi
    got = hostapi.learn_curve(8, 16, [64, 64], 3, 4, 2, 2e-3, 0.2, seed=5, nvec=(6, 6, 6), masked=True, n_playback=30, compute_dtype=1)
    assert got["forbidden_received"] == 0
    assert got["playback_actions"].shape == (30, 3) and np.all(got["playback_legal"] == 1.0)
    kc = got["kernel_counts"]
    only_new_names(kc, None, "<mcat,mask>")
    assert kc["bf16_step_sequence<mcat,mask>"] >= 3 * 16, kc      # (the value-only pass that closes a rollout takes no mask)


@gpu
def test_errors_and_flag_contract():
    import ctypes
    import ppo_cpp_amd
    Err = ppo_cpp_amd.PPOHipError
    O, nvec, hidden, n = 18, (3, 5), [256, 128], 40
    A = sum(nvec)
    multi = dict(action_dist="multi_categorical", nvec=list(nvec))
    with pytest.raises(Err, match="the multi-categorical head runs on the PPO_F32 path"):
        ppo_cpp_amd.PPOHip(O, None, hidden, compute_dtype=1, **multi)
    with pytest.raises(Err, match="at most 128"):
        ppo_cpp_amd.PPOHip(O, None, hidden, action_dist="multi_categorical", nvec=[65, 64], compute_dtype=1, bf16_head=True)
    rc, msg = create_multi_ex(list(nvec), 0x1000 | 0x800, compute_dtype=1)
    assert rc != 0 and "unknown flag bit 0x800" in msg, msg
    rc, msg = create_multi_ex(list(nvec), 0x200, compute_dtype=1)
    assert rc != 0 and "the multi-categorical head runs on the PPO_F32 path" in msg, msg
    assert create_multi_ex(list(nvec), 0x1000 | 0x100 | 0x400 | 0x200, compute_dtype=1) == (0, "")     # the other flags beside it: accepted
    lib = ppo_cpp_amd.load_library()
    h = ctypes.c_void_p()
    probe = ppo_cpp_amd.PPOHip(O, A, hidden)
    assert lib.ppo_create_ex(ctypes.byref(probe.cfg), 1 | 0x1000, ctypes.byref(h)) != 0 and b"unknown action_dist" in lib.ppo_last_error(None)
    assert lib.ppo_abi_version() == 3
    probe.close()
    obs, u, mask = inputs(O, nvec, n)
    ref = make_ref(hidden, O, nvec)

    def trace(g):
        g.set_flat(ref.theta.astype(np.float32))
        a, v, nlp = g.step(obs, u)
        losses = g.train_step(LR, CR, obs, a, np.linspace(-1, 1, n).astype(np.float32), v + 0.3, nlp + 0.05, v - 0.1)
        out = [a, v, nlp, losses, g.get_flat(0), g.kernel_counts(), g.lib.ppo_action_dist(g.h)]
        g.close()
        return out
    # the flag on a PPO_F32 handle: the bits and the counts of a handle without it (capi passes no flag there; the C entry point with the bit likewise)
    x, y = trace(ppo_cpp_amd.PPOHip(O, None, hidden, **multi)), trace(ppo_cpp_amd.PPOHip(O, None, hidden, bf16_head=True, **multi))
    z_g = ppo_cpp_amd.PPOHip(O, None, hidden, **multi)         # ... and its handle swapped for one from ppo_create_multi_ex(.., PPO_ACT_BF16_MULTI_HEAD, ..) itself
    hz = ctypes.c_void_p()
    nv = (ctypes.c_int32 * len(nvec))(*nvec)
    assert lib.ppo_create_multi_ex(ctypes.byref(z_g.cfg), nv, len(nvec), 0x1000, ctypes.byref(hz)) == 0
    lib.ppo_destroy(z_g.h); z_g.h = hz
    z = trace(z_g)
    for other in (y, z):
        for p, q in zip(x[:5], other[:5]):
            np.testing.assert_array_equal(p, q)
        assert x[5] == other[5] and x[6] == other[6] == 2, (x[5], other[5])
    assert x[5]["policy_step_kernel<mcat>"] == 1 and all(x[5][name] == 0 for name in NEW_NAMES)
    # PPO_ACT_SHAPE_KERNELS / PPO_ACT_PAIR_KERNELS beside the flag: accepted and ignored, the handle is a bf16 one
    g = ppo_cpp_amd.PPOHip(O, None, hidden, compute_dtype=1, bf16_head=True, shape_kernels=True, pair_kernels=True, **multi)
    g.step(obs)
    assert g.kernel_counts()["bf16_step_sequence<mcat>"] == 1 and g.lib.ppo_action_dist(g.h) == 2
    g.close()
    # data parallel: refused with the documented message, and the handle then still steps and trains
    g = ppo_cpp_amd.PPOHip(O, None, hidden, compute_dtype=1, bf16_head=True, ent_coef=ENT, **multi)
    g.set_flat(ref.theta.astype(np.float32))
    with pytest.raises(Err, match="data parallel is not supported for a multi-categorical PPO_BF16 handle created with PPO_ACT_BF16_MULTI_HEAD"):
        g.dist_init(1, 0, b"\0" * 128)
    a, v, nlp = g.step(obs, u, mask=mask)
    theta = g.get_flat(0)
    # host-side refusals before anything is trained: a component without an allowed category, an action out of its component's range
    none = mask.copy(); none[3, nvec[0]:] = 0
    with pytest.raises(Err, match="allows no category"):
        g.step(obs, u, mask=none)
    bad = a.copy(); bad[2, 1] = nvec[1]
    with pytest.raises(Err):
        g.train_step(LR, CR, obs, bad, v, v, nlp, v)
    np.testing.assert_array_equal(g.get_flat(0), theta)
    assert g.kernel_counts()["bf16_train_sequence<mcat,mask>"] == 0 and g.kernel_counts()["bf16_train_sequence<mcat>"] == 0
    losses = g.train_step(LR, CR, obs, a, np.linspace(-1, 1, n).astype(np.float32), v + 0.3, nlp, v, mask=mask)
    assert np.isfinite(losses).all() and np.any(g.get_flat(0) != theta)
    # a checkpoint saved from the bf16 handle loads into an fp32 multi handle of the same nvec, and the reverse.  The library has no file entry point of its own: the
    # project's checkpoint is PPO2::save / PPO2::load, which move the named tensors through ppo_get_tensor / ppo_set_tensor (and the components through the side-car,
    # compared with ppo_action_nvec).  First those calls, tensor by tensor, both ways; then the whole training state (flat weights, both Adam slots, the beta powers)
    gs = ppo_cpp_amd.PPOHip(O, None, hidden, ent_coef=ENT, **multi)
    assert gs.tensors == g.tensors and gs.nvec == g.nvec
    gs.set_tensors({name: g.get_tensor(name) for name, _ in g.tensors})           # bf16 -> fp32
    np.testing.assert_array_equal(gs.get_flat(0), g.get_flat(0))
    gs.train_step(LR, CR, obs, a, np.linspace(-1, 1, n).astype(np.float32), v + 0.3, nlp, v, mask=mask)
    gl = ppo_cpp_amd.PPOHip(O, None, hidden, compute_dtype=1, bf16_head=True, ent_coef=ENT, **multi)
    gl.set_tensors({name: gs.get_tensor(name) for name, _ in gs.tensors})         # fp32 -> bf16: the operand mirror follows the upload
    np.testing.assert_array_equal(gl.get_flat(0), gs.get_flat(0))
    gfresh = ppo_cpp_amd.PPOHip(O, None, hidden, compute_dtype=1, bf16_head=True, ent_coef=ENT, **multi)
    gfresh.set_flat(gs.get_flat(0))
    for p, q in zip(gl.step(obs, u, mask=mask), gfresh.step(obs, u, mask=mask)):
        np.testing.assert_array_equal(p, q)
    gs.close(); gl.close(); gfresh.close()
    gf = ppo_cpp_amd.PPOHip(O, None, hidden, ent_coef=ENT, **multi)
    assert gf.tensors == g.tensors and gf.P == g.P
    for which in range(3):
        gf.set_flat(g.get_flat(which), which)
        np.testing.assert_array_equal(gf.get_flat(which), g.get_flat(which))
    gf.set_beta_powers(g.beta_powers())
    np.testing.assert_array_equal(gf.beta_powers(), g.beta_powers())
    for name, _ in g.tensors:
        np.testing.assert_array_equal(gf.get_tensor(name), g.get_tensor(name))
    af, vf_, nf = gf.step(obs, u, mask=mask)
    gf.train_step(LR, CR, obs, af, np.linspace(-1, 1, n).astype(np.float32), vf_ + 0.3, nf, vf_, mask=mask)
    g2 = ppo_cpp_amd.PPOHip(O, None, hidden, compute_dtype=1, bf16_head=True, ent_coef=ENT, **multi)
    for h2 in (g, g2):                                         # the reverse, into the used handle and into a fresh one: the same bits afterwards
        for which in range(3):
            h2.set_flat(gf.get_flat(which), which)
        h2.set_beta_powers(gf.beta_powers())
    outs = [h2.step(obs, u, mask=mask) for h2 in (g, g2)]
    for p, q in zip(*outs):
        np.testing.assert_array_equal(p, q)
    for which in range(3):
        np.testing.assert_array_equal(g.get_flat(which), gf.get_flat(which))
    g.close(); g2.close(); gf.close()
