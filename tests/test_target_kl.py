"""Target-KL early stopping inside the update: ppo_set_target_kl / ppo_get_target_kl / ppo_update_applied, PPOHip.set_target_kl, PPO2::set_target_kl.

A train step whose approxkl (losses[3]) exceeds 1.5 * target_kl is not applied and ends its ppo_update; the decision is taken on the device, in adam_kernel.  The
reference is tests/target_kl_ref.py: the update as a manual minibatch loop over the oracle's pieces that stops before the Adam step.  Four handles: the generic
Gaussian (4,5), the narrow Gaussian (64,64), the (256,256) pair, and the narrow categorical (64,64) with 6 categories and action masks.  The stop forms of the
other discrete heads (narrow and pair, categorical and multi-categorical, plain and masked) are launched by the two test_discrete_stop_forms_* tests, which need no
reference: they compare bits with the handle itself.

Tolerances are those of tests/test_hip_parity.py::test_update_phase_matches_oracle (rows rtol 2e-4 / atol 2e-6, theta rtol 2e-4 / atol 5e-6, powers rtol 1e-5;
its second update: rows rtol 3e-4 / atol 3e-6).  The categorical reference is float64: its clipfrac column may differ by one row of the minibatch, as in
tests/test_narrow_categorical.py.  Where the reference stops is decided with a margin: every limit lies at least 5 % away from every approxkl of the run
(asserted on the reference side), so the device's fp32 sums take the same decision."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import oracle as o
from tests import target_kl_ref as R
from tests.masked_categorical_ref import MaskedCatRef, random_masks

CR = 0.16102319955825806
LR = 0.000393141177482903
GAMMA, LAM = 0.99, 0.95
E, T = 8, 16
B = E * T
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("PPO_HIP_NO_LAZY_ADAM", "PPO_HIP_NO_NARROW_EPOCH")     # the forms that end every train step in adam_kernel

CASES = ["generic", "narrow", "pair", "narrow_cat_mask"]
HIDDEN = {"generic": (4, 5), "narrow": (64, 64), "pair": (256, 256), "narrow_cat_mask": (64, 64)}


def make_perms(epochs, seed=99):
    rng = np.random.RandomState(seed)
    perm = np.arange(B, dtype=np.int32); perms = []
    for _ in range(epochs):
        rng.shuffle(perm); perms.append(perm.copy())
    return np.stack(perms)


class Case:
    """one handle kind: the reference (fresh, CPU), its rollout, and what the GPU side needs to mirror it"""

    def __init__(self, name):
        self.name, self.hidden, self.cat, self.lr = name, HIDDEN[name], name == "narrow_cat_mask", LR
        self.ref = self.new_ref()
        if self.cat:
            from tests.test_action_mask import ref_rollout
            rng = np.random.RandomState(5)
            u = rng.uniform(size=(T, E, 6)).astype(np.float32)
            masks = random_masks(rng, T * E, 6, special=False).reshape(T, E, 6)
            ro = ref_rollout(self.ref, 500, E, T, u, masks)
            self.fields = R.FIELDS + ("masks",)
        else:
            noise = np.random.RandomState(23).normal(size=(T, E, 18)).astype(np.float32)
            ro, _, _ = o.collect(self.ref, o.Normalizer(E, 18), 1234, T, noise, GAMMA, LAM)
            self.fields = R.FIELDS
        self.ro = {f: np.asarray(ro[f], np.float32) for f in self.fields}

    def new_ref(self):
        if self.cat:
            ref = MaskedCatRef(18, 6, self.hidden)
            ref.init_random(1, 1.0)
            return ref
        orc = o.Oracle(18, 18, list(self.hidden))
        orc.init_orthogonal(3)
        orc.tensor("pi/logstd")[:] = np.random.RandomState(4).uniform(-1.0, 0.2, (1, 18))
        return orc

    def ref_update(self, ref, perms, nmb, limit=None, ro=None):
        fn = R.categorical_update if self.cat else R.gaussian_update
        return fn(ref, ro if ro is not None else self.ro, perms, nmb, self.lr, CR, limit)

    def ref_state(self, ref):
        return np.asarray(ref.theta, np.float64), np.asarray(ref.pow, np.float64)

    def clone(self, ref):
        """a reference with the same weights, Adam slots and beta powers"""
        r = self.new_ref()
        r.theta[:] = ref.theta; r.m[:] = ref.m; r.v[:] = ref.v
        r.pow = np.array(ref.pow, np.float32) if not self.cat else list(ref.pow)
        return r

    def handle(self):
        import ppo_cpp_amd
        if self.cat:
            g = ppo_cpp_amd.PPOHip(18, 6, list(self.hidden), action_dist="categorical", shape_kernels=True)
            c = g.cfg
            fresh = self.new_ref()
            assert (c.ent_coef, c.vf_coef, c.max_grad_norm) == (np.float32(fresh.ent), np.float32(fresh.vfc), np.float32(fresh.maxn))
            g.set_action_masking(True)
        else:
            g = ppo_cpp_amd.PPOHip(18, 18, list(self.hidden))
        g.set_flat(np.asarray(self.new_ref().theta, np.float32))
        g.norm_init(E)
        g.rollout_alloc(E, T)
        self.upload(g, self.ro)
        return g

    def upload(self, g, ro):
        for f in self.fields:
            g.rollout_set(f, ro[f])

    def fresh_obs(self):
        rng = np.random.RandomState(77)
        obs = rng.uniform(-1, 1, (40, 18)).astype(np.float32)
        mask = random_masks(rng, 40, 6, special=False) if self.cat else None
        return obs, mask


_CASES = {}


def case(name):
    """the reference rollout of a case is computed once and shared (never modified: every test copies what it changes)"""
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


_FREE_RUNS = {}


def free_run(name, epochs, nmb):
    """the reference's rows of an update without a limit (computed once per shape)"""
    key = (name, epochs, nmb)
    if key not in _FREE_RUNS:
        c = case(name)
        rows, applied = c.ref_update(c.new_ref(), make_perms(epochs), nmb)
        assert applied == epochs * nmb
        _FREE_RUNS[key] = rows
    return _FREE_RUNS[key]


def stop_point(name, epochs, nmb, min_s=2, allow_epoch_boundary=False):
    kl = free_run(name, epochs, nmb)[:, 3]
    pick = R.pick_limit(kl, nmb, min_s, allow_epoch_boundary)
    assert pick is not None, "the reference run has no step to stop at with a clear margin: %r" % (kl,)
    s, limit = pick
    assert s >= min_s and kl[s] > 1.05 * kl[:s].max() and R.clear_of(kl, limit), (s, limit, kl)
    return s, limit


def third_update_limit(c, ref):
    """the replay test's third update takes another limit: one at which the reference, continued from `ref` (not modified), trains again and stops at s3 >= 1"""
    rows, _ = c.ref_update(c.clone(ref), make_perms(3), 4)
    pick = R.pick_limit(rows[:, 3], 4, min_s=1, allow_epoch_boundary=True)
    assert pick is not None, rows[:, 3]
    return pick


def state(g):
    return {"theta": g.get_flat(0), "m": g.get_flat(1), "v": g.get_flat(2), "pow": g.beta_powers()}


def same_bits(a, b, msg):
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32), err_msg="%s: %s" % (msg, k))


def check_rows(c, rows, ref_rows, nmb, rtol=2e-4, atol=2e-6, msg=""):
    ncol = 4 if c.cat else 5
    np.testing.assert_allclose(rows[:, :ncol], ref_rows[:, :ncol], rtol=rtol, atol=atol, err_msg=msg)
    if c.cat:                                                             # (float64 reference: one row of the minibatch may sit on the other side of the clip range)
        assert np.all(np.abs(rows[:, 4] - ref_rows[:, 4]) <= nmb / B + 1e-6), msg


# ---- not-GPU ------------------------------------------------------------------------------------------------------------
def test_reference_loop_without_a_limit_is_the_oracles_update():
    """validates tests/target_kl_ref.py itself: with no limit it reproduces Oracle.update's rows and weights (bit for bit: the same C pieces in the same order)"""
    c = case("generic")
    perms = make_perms(3)
    a, b = c.new_ref(), c.new_ref()
    ref_rows, ref_mean = a.update(c.ro, perms, 4, c.lr, CR)
    rows, applied = R.gaussian_update(b, c.ro, perms, 4, c.lr, CR)
    assert applied == 12
    np.testing.assert_array_equal(rows, ref_rows)
    np.testing.assert_array_equal(b.theta, a.theta)
    np.testing.assert_array_equal(b.m, a.m); np.testing.assert_array_equal(b.v, a.v); np.testing.assert_array_equal(b.pow, a.pow)
    # ... and the categorical loop reproduces MaskedCatRef.update
    c = case("narrow_cat_mask")
    a, b = c.new_ref(), c.new_ref()
    ref_rows, _ = a.update(dict(c.ro), perms, 4, c.lr, CR)
    rows, applied = R.categorical_update(b, c.ro, perms, 4, c.lr, CR)
    assert applied == 12
    np.testing.assert_allclose(rows, ref_rows, rtol=1e-12, atol=0)
    np.testing.assert_allclose(b.theta, a.theta, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", CASES)
def test_reference_stops_with_a_clear_margin(name):
    """the seeds of the GPU cases: every run has a stop point s >= 2 inside an epoch whose limit lies 5 % clear of every approxkl, the stopped reference returns
    rows 0..s and applied s Adam steps, and the update after it (the replay test) is just as clear of the limit"""
    c = case(name)
    s, limit = stop_point(name, 3, 4)
    ref = c.new_ref()
    rows, applied = c.ref_update(ref, make_perms(3), 4, limit)
    assert applied == s and len(rows) == s + 1 and rows[s, 3] > limit
    np.testing.assert_array_equal(rows, free_run(name, 3, 4)[:s + 1])
    rows2, applied2 = c.ref_update(ref, make_perms(3), 4, limit)
    assert R.clear_of(rows2[:, 3], limit), (limit, rows2[:, 3])
    assert len(rows2) == applied2 + (1 if applied2 < 12 else 0)
    s3, limit3 = third_update_limit(c, ref)
    assert s3 >= 1 and limit3 > limit
    s1, _ = stop_point(name, 4, 1, min_s=2, allow_epoch_boundary=True)
    assert s1 >= 1


def test_symbols_header_and_struct():
    from ppo_cpp_amd import build, hostapi
    hdr = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert re.search(r"int ppo_set_target_kl\(ppo_handle\* h, float target_kl\);", hdr)
    assert re.search(r"int ppo_get_target_kl\(const ppo_handle\* h, float\* target_kl\);", hdr)
    assert re.search(r"int ppo_update_applied\(ppo_handle\* h, int32_t\* applied, int32_t\* total\);", hdr)
    build.build_all()
    lib = ctypes.CDLL(build.HIP_SO)
    for sym in ("ppo_set_target_kl", "ppo_get_target_kl", "ppo_update_applied"):
        assert hasattr(lib, sym), sym
    assert lib.ppo_abi_version() == 3
    assert lib.ppo_set_target_kl(None, ctypes.c_float(0.01)) != 0        # a null handle is an error, not a crash
    host = hostapi.load_host_library(build=False)
    assert host.ppo_host_args_size() == ctypes.sizeof(hostapi.HostArgs)
    assert host.ppo_host_explicit_size() == ctypes.sizeof(hostapi.HostExplicit)
    assert hostapi.HostExplicit._fields_[-1][0] == "target_kl"          # appended at the end of the struct the setting travels in
    assert hasattr(host, "ppo_host_target_kl_checkpoint")


def test_driver_help_names_target_kl():
    import subprocess
    from ppo_cpp_amd import build
    build.build_all()
    driver = os.path.join(ROOT, "ppo_cpp_amd", "ppo_cpp_hip")
    out = subprocess.run([driver, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--target_kl" in out.stdout
    bad = subprocess.run([driver, "--target_kl", "-1"], capture_output=True, text=True)
    assert bad.returncode == 1 and "--target_kl" in bad.stderr


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_stops_where_the_reference_stops_and_replays(name):
    """tests 1 and 5 of the issue: the first update stops at the reference's step s; the second one (a replay of the captured graph) starts with the stop
    condition cleared and trains on as the reference does; a changed target_kl is honoured by the next replay without a re-capture."""
    c = case(name)
    nmb, epochs = 4, 3
    perms = make_perms(epochs)
    s, limit = stop_point(name, epochs, nmb)
    ref = c.new_ref()
    ref_rows, ref_applied = c.ref_update(ref, perms, nmb, limit)
    g = c.handle()
    g.set_target_kl(limit / 1.5)
    # the limit the library forms is 1.5f * target_kl: within an ulp or two of `limit`, far inside the 5 % margin
    assert abs(np.float32(1.5) * np.float32(g.target_kl()) - np.float32(limit)) <= 4e-7 * limit
    rows, mean = g.update(c.lr, CR, epochs, nmb, perms)
    print("approxkl", rows[:, 3], "limit", limit, "reference", ref_rows[:, 3])
    assert g.update_applied() == (s, epochs * nmb) == (ref_applied, 12)
    check_rows(c, rows[:s + 1], ref_rows, nmb, msg="rows 0..s")
    assert np.all(np.isnan(rows[s + 1:])), rows[s + 1:]
    assert rows[s, 3] > np.float32(1.5) * np.float32(g.target_kl()) and np.all(rows[:s, 3] <= np.float32(1.5) * np.float32(g.target_kl()))
    np.testing.assert_allclose(mean, rows[:s + 1].astype(np.float64).mean(0), rtol=1e-6, atol=1e-9)
    theta, pw = c.ref_state(ref)
    np.testing.assert_allclose(g.get_flat(0), theta, rtol=2e-4, atol=5e-6, err_msg="theta")
    np.testing.assert_allclose(g.beta_powers(), pw, rtol=1e-5)
    grad, norm = g.last_grad()                                           # the gradient and norm of step s (the reference's step s, before its clip)
    assert np.isfinite(norm) and norm > 0 and np.isclose(np.sqrt(np.dot(grad.astype(np.float64), grad.astype(np.float64))), norm, rtol=1e-4)
    nodes = g.debug_graph_nodes()
    assert nodes is not None and nodes["kernel"] > 0 and nodes["memset"] == 0 and nodes["memcpy"] == 0 and nodes["other"] == 0, nodes
    kc = g.kernel_counts()
    if name == "narrow":
        assert kc["narrow_train_kernel<static>"] + kc["narrow_train_kernel<runtime>"] == 12 and kc["narrow_epoch_kernel"] == 0, kc
    if name == "narrow_cat_mask":
        assert kc["narrow_train_kernel<cat,mask>"] == 12 and kc["narrow_epoch_kernel"] == 0, kc
    # the next update: a replay; the stop condition is cleared
    ref_rows2, ref_applied2 = c.ref_update(ref, perms, nmb, limit)
    assert R.clear_of(ref_rows2[:, 3], limit)
    rows2, mean2 = g.update(c.lr, CR, epochs, nmb, perms)
    print("second update: approxkl", rows2[:, 3], "reference", ref_rows2[:, 3])
    assert g.update_applied() == (ref_applied2, 12)
    n2 = len(ref_rows2)
    check_rows(c, rows2[:n2], ref_rows2, nmb, rtol=3e-4, atol=3e-6, msg="second update")
    assert np.all(np.isnan(rows2[n2:]))
    np.testing.assert_allclose(mean2, rows2[:n2].astype(np.float64).mean(0), rtol=1e-6, atol=1e-9)
    # a changed target_kl between replays: honoured -- the update trains again and stops where the reference, continued, stops under the new limit -- and nothing
    # was captured again (the host code of a train step does not run on a replay: the counts stand)
    s3, limit3 = third_update_limit(c, ref)
    g.set_target_kl(limit3 / 1.5)
    ref_rows3, ref_applied3 = c.ref_update(ref, perms, nmb, limit3)
    rows3, _ = g.update(c.lr, CR, epochs, nmb, perms)
    print("third update: approxkl", rows3[:, 3], "limit", limit3, "reference", ref_rows3[:, 3])
    assert ref_applied3 == s3 >= 1 and g.update_applied() == (s3, 12)
    check_rows(c, rows3[:s3 + 1], ref_rows3, nmb, rtol=3e-4, atol=3e-6, msg="third update")
    assert np.all(np.isnan(rows3[s3 + 1:]))
    assert g.kernel_counts() == kc
    nodes = g.debug_graph_nodes()
    assert nodes["kernel"] > 0 and nodes["memset"] == 0 and nodes["memcpy"] == 0 and nodes["other"] == 0, nodes
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_a_skipped_step_applies_nothing(name):
    """test 2: neglogp + 0.1 puts step 0 over the limit (approxkl = 0.005 against 0.0015).  Weights, Adam slots, beta powers and what the act side computes are
    bitwise what they were -- after one ordinary update, so that the slots are not zeros -- through ppo_update and through ppo_train_step."""
    c = case(name)
    nmb, epochs = 4, 3
    perms = make_perms(epochs)
    g = c.handle()
    g.update(c.lr, CR, 1, nmb, perms[:1])                               # an ordinary update first (setting off)
    assert g.update_applied() == (4, 4)
    obs, mask = c.fresh_obs()
    act = (lambda: g.act_deterministic(obs, mask)) if c.cat else (lambda: g.act_deterministic(obs))
    before, v0, a0 = state(g), g.value(obs), act()
    assert np.abs(before["m"]).max() > 0 and np.abs(before["v"]).max() > 0
    ro = dict(c.ro); ro["neglogp"] = (c.ro["neglogp"] + np.float32(0.1)).astype(np.float32)
    c.upload(g, ro)
    g.set_target_kl(0.001)
    rows, mean = g.update(c.lr, CR, epochs, nmb, perms)
    assert g.update_applied() == (0, 12)
    assert np.all(np.isfinite(rows[0])) and rows[0, 3] > 0.0015 and np.all(np.isnan(rows[1:])), rows
    np.testing.assert_array_equal(mean, rows[0])
    same_bits(before, state(g), "after the stopped update")
    np.testing.assert_array_equal(g.value(obs).view(np.uint32), v0.view(np.uint32))
    np.testing.assert_array_equal(act().view(np.uint32), a0.view(np.uint32))
    # the same through ppo_train_step: the first minibatch of the first epoch
    sl = next(R.minibatches(ro, perms, nmb, c.fields))
    adv = o.adv_normalize(sl["returns"], sl["values"])
    args = (c.lr, CR, sl["obs"], sl["actions"], adv, sl["returns"], sl["neglogp"], sl["values"])
    losses = g.train_step(*args, mask=sl["masks"]) if c.cat else g.train_step(*args)
    assert g.update_applied() == (0, 1)
    assert np.all(np.isfinite(losses)) and losses[3] > 0.0015
    np.testing.assert_allclose(losses[:4], rows[0, :4], rtol=2e-4, atol=2e-6)     # (the same minibatch; advantages normalised by the oracle here, on the device there)
    same_bits(before, state(g), "after the skipped train step")
    np.testing.assert_array_equal(g.value(obs).view(np.uint32), v0.view(np.uint32))
    # ... and with the setting off the same call is applied
    g.set_target_kl(0.0)
    g.train_step(*args, mask=sl["masks"]) if c.cat else g.train_step(*args)
    assert g.update_applied() == (1, 1)
    assert not np.array_equal(g.get_flat(0), before["theta"])
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_applied_steps_are_the_ordinary_steps(name, monkeypatch):
    """tests 3 and 4.  nmb = 1, 4 epochs, a limit that stops at s >= 1: the state is bitwise that of a fresh handle with the setting off that ran the first s
    epochs under PPO_HIP_NO_LAZY_ADAM=1 + PPO_HIP_NO_NARROW_EPOCH=1, and rows 0..s-1 are its rows.  A limit that never triggers (target_kl = 1e30) changes
    nothing: rows, mean and state are bitwise the setting-off run's under the same switches."""
    c = case(name)
    perms = make_perms(4)
    s, limit = stop_point(name, 4, 1, min_s=2, allow_epoch_boundary=True)
    g = c.handle()                                                       # (created without the switches: the setting alone selects the forms)
    g.set_target_kl(limit / 1.5)
    rows, _ = g.update(c.lr, CR, 4, 1, perms)
    print("approxkl", rows[:, 3], "limit", limit, "s", s)
    assert g.update_applied() == (s, 4)
    got = state(g)
    g.close()
    for sw in SWITCHES:
        monkeypatch.setenv(sw, "1")
    plain = c.handle()
    assert plain.target_kl() == 0.0
    ref_rows, _ = plain.update(c.lr, CR, s, 1, perms[:s])
    assert plain.update_applied() == (s, s)
    same_bits(got, state(plain), "stopped at s against s ordinary steps")
    np.testing.assert_array_equal(rows[:s].view(np.uint32), ref_rows.view(np.uint32))
    plain.close()
    # a limit that never triggers
    perms12 = make_perms(3)
    off = c.handle()
    rows_off, mean_off = off.update(c.lr, CR, 3, 4, perms12)
    on = c.handle()
    on.set_target_kl(1e30)
    rows_on, mean_on = on.update(c.lr, CR, 3, 4, perms12)
    assert on.update_applied() == (12, 12) and off.update_applied() == (12, 12)
    np.testing.assert_array_equal(rows_on.view(np.uint32), rows_off.view(np.uint32))
    np.testing.assert_array_equal(mean_on.view(np.uint32), mean_off.view(np.uint32))
    same_bits(state(on), state(off), "a limit that never triggers")
    on.close(); off.close()


# ---- the stop forms of the discrete heads: bits against the handle itself, no reference model -----------------------------------------
HEAD_E, HEAD_T, HEAD_EPOCHS, HEAD_NMB = 16, 4, 2, 2
HEAD_NVEC = (3, 5, 4, 6)
HEAD_FAMILIES = {"narrow": ((64, 64), "shape_kernels", "narrow_train_kernel"), "pair": ((256, 256), "pair_kernels", "train8_kernel")}
HEAD_FORMS = {"cat": ("categorical", False), "cat_mask": ("categorical", True), "mcat": ("multi_categorical", False), "mcat_mask": ("multi_categorical", True)}
HEAD_CASES = [f + "_" + h for f in HEAD_FAMILIES for h in HEAD_FORMS if f + "_" + h != "narrow_cat_mask"]       # (narrow_cat_mask: CASES above)
_HEAD_ROLLOUTS = {}


def head_handle(name):
    """a fresh handle of the case with its rollout uploaded: rows from a fixed RandomState, actions / values / neglogp from the handle's own act model
    (computed once per case and shared: every handle of a case starts from the same weights)"""
    import ppo_cpp_amd
    family, form = name.split("_", 1)
    hidden, flag, _ = HEAD_FAMILIES[family]
    dist, masked = HEAD_FORMS[form]
    g = ppo_cpp_amd.PPOHip(18, 18, list(hidden), action_dist=dist, nvec=HEAD_NVEC if dist == "multi_categorical" else None, **{flag: True})
    g.init_orthogonal(0)
    if masked:
        g.set_action_masking(True)
    g.norm_init(HEAD_E)
    g.rollout_alloc(HEAD_E, HEAD_T)
    if name not in _HEAD_ROLLOUTS:
        rng = np.random.RandomState(31)
        n = HEAD_E * HEAD_T
        obs = rng.normal(size=(n, 18)).astype(np.float32)
        mask = None
        if masked:
            mask = (rng.uniform(size=(n, 18)) < 0.6).astype(np.float32)
            mask[:, np.cumsum((0,) + HEAD_NVEC[:-1])] = 1.0                 # an open category in every component (and in the single one)
        act, val, nlp = g.step(obs, rng.uniform(0.01, 0.99, (n, 18)).astype(np.float32), mask=mask)
        ro = {"obs": obs, "actions": act, "values": val, "neglogp": nlp, "returns": (val + rng.normal(size=n) * 0.1).astype(np.float32)}
        if masked:
            ro["masks"] = mask
        _HEAD_ROLLOUTS[name] = {k: np.ascontiguousarray(v.reshape((HEAD_T, HEAD_E) + v.shape[1:])) for k, v in ro.items()}
    for f, v in _HEAD_ROLLOUTS[name].items():
        g.rollout_set(f, v)
    return g


def head_count(g, name):
    family, form = name.split("_", 1)
    return g.kernel_counts()["%s<%s>" % (HEAD_FAMILIES[family][2], form.replace("_", ","))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", HEAD_CASES)
def test_discrete_stop_forms_apply_the_ordinary_steps(name):
    """a limit that never triggers (target_kl = 1e30) launches the *_stop_kernel forms of the head and leaves weights, Adam slots and beta powers bitwise those
    of a fresh handle with the setting off that ran the same update"""
    total = HEAD_EPOCHS * HEAD_NMB
    off = head_handle(name)
    rows_off, _ = off.update(LR, CR, HEAD_EPOCHS, HEAD_NMB, seed=5)
    on = head_handle(name)
    on.set_target_kl(1e30)
    rows_on, _ = on.update(LR, CR, HEAD_EPOCHS, HEAD_NMB, seed=5)
    assert on.update_applied() == (total, total) and off.update_applied() == (total, total)
    assert head_count(on, name) == total and head_count(off, name) == total, on.kernel_counts()      # (the flag took effect: the family's own train kernel ran)
    assert not np.array_equal(off.get_flat(0), head_handle_theta0(name))
    same_bits(state(on), state(off), "a limit that never triggers")
    np.testing.assert_array_equal(rows_on.view(np.uint32), rows_off.view(np.uint32))
    on.close(); off.close()


def head_handle_theta0(name):
    g = head_handle(name)
    theta = g.get_flat(0)
    g.close()
    return theta


@pytest.mark.gpu
@pytest.mark.parametrize("name", HEAD_CASES)
def test_discrete_stop_forms_skip_a_step(name):
    """the old neglogp shifted by 0.1 (approxkl = 0.005 against a limit of 0.0015), as in test_a_skipped_step_applies_nothing: after one ordinary update, so that
    the slots are not zeros, the stopped update changes nothing bitwise and reports 0 applied steps"""
    total = HEAD_EPOCHS * HEAD_NMB
    g = head_handle(name)
    g.update(LR, CR, 1, HEAD_NMB, seed=5)
    assert g.update_applied() == (HEAD_NMB, HEAD_NMB)
    before = state(g)
    assert np.abs(before["m"]).max() > 0 and np.abs(before["v"]).max() > 0
    g.rollout_set("neglogp", (_HEAD_ROLLOUTS[name]["neglogp"] + np.float32(0.1)).astype(np.float32))
    g.set_target_kl(0.001)
    rows, _ = g.update(LR, CR, HEAD_EPOCHS, HEAD_NMB, seed=5)
    print(name, "approxkl", rows[:, 3])
    assert g.update_applied() == (0, total)
    assert np.all(np.isfinite(rows[0])) and rows[0, 3] > 0.0015 and np.all(np.isnan(rows[1:])), rows
    assert head_count(g, name) == HEAD_NMB + total, g.kernel_counts()
    same_bits(before, state(g), "after the stopped update")
    g.close()


@pytest.mark.gpu
def test_refusals_and_validation():
    import ppo_cpp_amd
    g = ppo_cpp_amd.PPOHip(18, 18, [64, 64])
    assert g.target_kl() == 0.0 and g.update_applied() == (0, 0)
    g.set_target_kl(0.02)
    for bad in (-0.01, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ppo_cpp_amd.PPOHipError, match="ppo_set_target_kl: needs a finite value >= 0"):
            g.set_target_kl(bad)
        assert g.target_kl() == np.float32(0.02)                        # the previous setting is kept
    # ppo_dist_init with the setting on: refused, the handle stays usable
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="ppo_dist_init: data parallel is not supported with target-KL early stopping on"):
        g.dist_init(1, 0, bytes(128))
    g.set_target_kl(0.0)
    g.dist_init(1, 0, ppo_cpp_amd.PPOHip.dist_unique_id())              # a one-rank communicator
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="ppo_set_target_kl: not supported on a data-parallel handle"):
        g.set_target_kl(0.02)
    assert g.target_kl() == 0.0
    g.set_target_kl(0.0)                                                 # off is always accepted
    g.close()
    b = ppo_cpp_amd.PPOHip(18, 18, [256, 256], compute_dtype=1)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="ppo_set_target_kl: not supported on a PPO_BF16 handle"):
        b.set_target_kl(0.02)
    assert b.target_kl() == 0.0
    b.set_target_kl(0.0)
    b.close()


@pytest.mark.gpu
def test_host_layer(tmp_path):
    """test 7: PPO2::set_target_kl through learn_curve at E=4, T=16 -- the resident loop (ppo_update) and the reference loop (ppo_train_step per minibatch) stop
    after the same number of steps in the first update; the checkpoint side-car round-trips target_kl and one without the key loads as off."""
    from ppo_cpp_amd import hostapi
    # one minibatch per epoch: the two loops shuffle differently (on the device / std::shuffle), and with nminibatches = 1 every train step sees the whole batch
    # whatever the order, so both compute the same approxkl sequence up to the rounding of the sums
    EP = 12
    kw = dict(n_envs=4, n_steps=16, hidden=[64, 64], nminibatches=1, lr=3e-3, cliprange=0.2, seed=5)
    # the first update's approxkl, step by step, from free runs of 1 .. EP epochs (seeded: each is a prefix of the next): row n - 1 = n mean_n - (n - 1) mean_{n-1}
    frees = [hostapi.learn_curve(n_updates=1, noptepochs=n, **kw) for n in range(1, EP + 1)]
    sums = np.array([0.0] + [n * float(f["losses"][0, 3]) for n, f in zip(range(1, EP + 1), frees)])
    kl = np.diff(sums)
    free = frees[-1]
    assert tuple(free["applied"][0]) == (EP, EP)
    # the limit: with the 5 % clearance of the update tests, so that the two loops' differently ordered sums take the same decision
    pick = R.pick_limit(kl, 1, min_s=2, allow_epoch_boundary=True)
    assert pick is not None, kl
    s, limit = pick
    assert kl[s] > 1.05 * kl[:s].max() and R.clear_of(kl, limit), (s, limit, kl)
    target = limit / 1.5
    res = hostapi.learn_curve(target_kl=target, n_updates=2, noptepochs=EP, **kw)
    lit = hostapi.learn_curve(target_kl=target, reference_loop=True, n_updates=2, noptepochs=EP, **kw)
    print("approxkl", kl, "limit", limit, "applied", res["applied"], lit["applied"])
    assert tuple(res["applied"][0]) == (s, EP)
    assert tuple(lit["applied"][0]) == (s, EP)
    np.testing.assert_allclose(res["losses"][0], lit["losses"][0], rtol=2e-3, atol=1e-5)
    np.testing.assert_allclose(res["losses"][0, 3], kl[:s + 1].mean(), rtol=1e-3)
    assert res["kernel_counts"]["narrow_epoch_kernel"] == 0 and free["kernel_counts"]["narrow_epoch_kernel"] > 0
    assert hostapi.target_kl_checkpoint(str(tmp_path / "a"), 0.03) == np.float32(0.03)
    assert hostapi.target_kl_checkpoint(str(tmp_path / "b"), 0.03, strip_key=True) == 0.0
    assert hostapi.target_kl_checkpoint(str(tmp_path / "c"), 0.0) == 0.0
