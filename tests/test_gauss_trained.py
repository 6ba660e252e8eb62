"""The fp32 Gaussian path at trained-looking weights, in every kernel family: one act call of each kind, one three-step collect and one train step per kernel against
the float64 reference (oracle/torch_check.py).  Inputs, the fp32 emulation, the bounds and the fault models are in tests/gauss_trained_ref.py, which says what they
are and why the regime matters.

CPU tests: the conditions on the inputs at every shape and row count used below; the emulation at float64 IS the reference's losses and gradient; the fp32
emulation passes every assertion, also with the rows reversed and every row's neglogp one float32 up or down; each fault model is rejected by its named assertion
at trained weights, the first four are accepted by the `orth` control (the regime every other test runs in), dy_bf16 is rejected by the per-tensor L2 rule at both
weight sets; the MEASURED guard.
GPU tests (skipped without a device), every case once at trained weights and once at the control:
    act      step (explicit noise), value, act_deterministic, evaluate_actions: mu, value, action, neglogp, entropy; the kernel_counts() delta is exactly three launches
             of the case's step kernel (policy_eval_kernel, which serves evaluate_actions, has no row there: a fall-back to a counted kernel shows as a fourth launch)
    rollout  collect_synthetic(T = 3, explicit noise) behind set_norm_stats; mu, value and neglogp recomputed in float64 from the device's own stored observations
             (teacher forcing: tests/test_envnorm_trained.py owns the normaliser); the delta is the same-named entry of tests/golden/rollout_forms.json
    train    one train_step, then last_grad() and get_flat(0..2): losses, gradient (elementwise and per tensor), norm, theta, Adam m and v; the delta is the form's
(16, 8, 8) qualifies for the narrow family: its cases run under PPO_HIP_NO_NARROW=1, which is how the suite reaches the generic kernels with three layers.

One fault of the issue's list was replaced: clip_pass_dropped restores the whole unclipped gradient on EVERY clipped row (pass is 0 exactly where the clipped
branch is selected), so the control, whose clip fraction is 0.2 to 0.4, rejects it at every shape; ratio_exp_clamped (the ratio's exponent clamped to +-4) shows
only on rows deep in the clip.  test_fault_table asserts both halves of that statement.
"""
import functools
import json

import numpy as np
import pytest

from tests import gauss_trained_ref as R

CR, LR = R.CR, R.LR
GAMMA, LAM = 0.99, 0.95
KINDS = ("trained", "orth")

# (id, hidden, O, A, rows, switches set to 1, the step kernel)
ACT_CASES = [
    ("static_n1", (64, 64), 18, 18, 1, (), "narrow_step_kernel<static>"),
    ("static_n33", (64, 64), 18, 18, 33, (), "narrow_step_kernel<static>"),
    ("runtime_32_32", (32, 32), 18, 18, 33, (), "narrow_step_kernel<runtime>"),
    ("runtime_o20_a40", (64, 64), 20, 40, 33, (), "narrow_step_kernel<runtime>"),
    ("generic_o80", (64, 64), 80, 18, 17, (), "policy_step_kernel"),
    ("generic_16_8_8", (16, 8, 8), 18, 18, 17, ("PPO_HIP_NO_NARROW",), "policy_step_kernel"),
    ("pair_n16", (256, 256), 18, 18, 16, (), "policy_step_kernel"),
    ("pair_n80", (256, 256), 18, 18, 80, (), "policy_step_kernel"),                 # past four row blocks
    ("pair_o36_a40_n16", (256, 256), 36, 40, 16, (), "policy_step_kernel"),
    ("pair_o36_a40_n80", (256, 256), 36, 40, 80, (), "policy_step_kernel"),
]
GENERIC = {"grad_reduce_kernel": 1, "train_fwd_bwd_kernel": 1, "weight_grad_kernel": 1}
PAIR = {"train8_kernel": 1, "weight_grad_assemble_kernel": 1}
# (id, hidden, O, A, rows, switches set to 1, the kernel_counts() delta of one train step)
TRAIN_CASES = [
    ("static_n33", (64, 64), 18, 18, 33, (), {"narrow_train_kernel<static>": 1}),
    ("static_n64", (64, 64), 18, 18, 64, (), {"narrow_train_kernel<static>": 1}),
    ("runtime_32_32", (32, 32), 18, 18, 33, (), {"narrow_train_kernel<runtime>": 1}),
    ("runtime_o20_a40", (64, 64), 20, 40, 33, (), {"narrow_train_kernel<runtime>": 1}),
    ("generic_o80", (64, 64), 80, 18, 17, (), GENERIC),
    ("generic_16_8_8", (16, 8, 8), 18, 18, 17, ("PPO_HIP_NO_NARROW",), GENERIC),
    ("pair_n40", (256, 256), 18, 18, 40, (), PAIR),                                 # live, half-dead and dead tiles
    ("pair_o36_a40_n40", (256, 256), 36, 40, 40, (), PAIR),
    ("pair_n576", (256, 256), 18, 18, 576, (), PAIR),                               # nine 64-row chunks, which the four splits own as 2, 2, 2 and 3
    ("pair_no_t8_n100", (256, 256), 18, 18, 100, ("PPO_HIP_NO_T8",), GENERIC),
    ("pair_no_dw2_n128", (256, 256), 18, 18, 128, ("PPO_HIP_NO_DW2",), {"grad_reduce_kernel": 1, "train8_kernel": 1, "weight_grad_kernel": 1}),
]
ROLLOUT_CASES = ("dev_e1", "dev_e1_no_rollout1", "dev_e8", "dev_e96", "dev_e8_no_persistent", "dev_256_e16")      # entries of tests/test_rollout_forms.CASES
SHAPES = sorted({c[1:5] for c in ACT_CASES + TRAIN_CASES})


@functools.lru_cache(maxsize=None)
def case(hidden, O, A, n, kind):
    """(batch, the float64 reference's train step or None for one row, bounds): computed once, shared by every test, left unchanged"""
    b = R.Batch(R.oracle_for(hidden, O, A), kind, n)
    if n == 1:
        return b, None, R.act_bounds(b)
    want = b.reference_step()
    return b, want, R.bounds(b, want)


def test_constants_are_the_projects_own():
    from tests import test_hip_parity as P
    from tests import head_edges_ref as E
    from tests import bf16_ref as B
    assert (R.CR, R.LR) == (P.CR, P.LR) and R.FACTOR == E.PART2_FACTOR == B.L2_FACTOR
    assert (GAMMA, LAM) == (P.GAMMA, P.LAM)


# =====================================================================================================================================================
# CPU: the inputs and the comparison's teeth
# =====================================================================================================================================================
@pytest.mark.parametrize("hidden,O,A,n", SHAPES, ids=lambda x: str(x).replace(" ", ""))
def test_input_conditions(hidden, O, A, n):
    """from the float64 forward alone.  A one-row case (the second row of a two-row draw) is held to the conditions a single row can meet."""
    b, want, _ = case(hidden, O, A, n, "trained")
    st = R.input_stats(b)
    print(hidden, O, A, n, st, "" if want is None else "clipfrac %.3f, clip edges %s" % (want["losses"][4], R.edge_distance(b.v, b.nlp_given, b.mb)))
    assert not st["zero_biases"], st["zero_biases"]
    assert np.all(b.theta == b.theta.astype(np.float32)) and b.theta.dtype == np.float32
    for x in (b.mu, b.v, b.nlp_given, b.nlp_sample):
        assert np.isfinite(x).all()
    if n == 1:
        assert np.any(b.obs != 0)
        return
    assert not np.any(b.obs[0]) and np.any(np.abs(b.obs) == 10.0)
    for tw, share in st["sat"].items():
        assert 0.05 <= share <= 0.6, (tw, share)
    assert st["poly"] >= 0.01, st["poly"]
    assert st["mu_max"] >= 1.0 and st["nlp_min"] < 0.0, st
    assert 0.02 < want["losses"][4] < 0.98
    assert min(R.edge_distance(b.v, b.nlp_given, b.mb)) >= b.band >= R.BAND, "a row lies inside the clip-edge band"
    assert b.band >= R.FACTOR * R.nlp_error(b, b.actions, b.nlp_given)
    for x in tuple(b.train_args()) + (want["losses"], want["grad"], want["theta"], want["m"], want["v"]):
        assert np.isfinite(x).all()
    # the forced rows: an eighth of the rows, the smallest |adv|, ratio e^+-5 with both signs, old_values 2 away with both signs
    f = b.forced
    assert f.sum() == n // 8 and np.abs(b.mb["advs"][f]).max() <= np.abs(b.mb["advs"][~f]).min()
    d = b.mb["old_neglogp"][f] - b.nlp_given[f]
    assert np.allclose(np.abs(d), R.FORCED_NLP, atol=1e-5) and (d > 0).any() and (d < 0).any()
    assert np.allclose(np.abs(b.mb["old_values"][f] - b.v[f]), R.FORCED_V, atol=1e-5)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hidden,O,A,n", [((64, 64), 18, 18, 33), ((64, 64), 20, 40, 33), ((16, 8, 8), 18, 18, 17), ((256, 256), 36, 40, 40)])
def test_emulation_at_float64_is_the_reference(hidden, O, A, n, kind):
    b, want, _ = case(hidden, O, A, n, kind)
    e = R.emulate(b.theta, b, np.float64)
    np.testing.assert_allclose(e["mu"], b.mu, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(e["v"], b.v, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(e["nlp"], b.nlp_given, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(e["ent"], b.ent_rows, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(e["losses"], want["losses"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(e["grad"], want["grad"], rtol=1e-9, atol=1e-9 * np.abs(want["grad"]).max())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hidden,O,A,n", SHAPES, ids=lambda x: str(x).replace(" ", ""))
def test_fp32_emulation_passes_every_assertion(hidden, O, A, n, kind):
    """... as computed, with the rows reversed, and with every row's neglogp one float32 up or down (seeds the bounds did not see)"""
    b, want, bnd = case(hidden, O, A, n, kind)
    assert not R.act_failures(b, R.emulated_act(b), bnd)
    if n == 1:
        return
    got = R.emulated_train(b)
    name, l2, bound = R.l2_report(b, got, want, bnd)
    print("%s %s n=%d %s: fp32 emulation under the elementwise rule alone %.2f, nearest L2 bound %s %.3g (%.3g)" % (hidden, (O, A), n, kind, R.usual_rule_ratio(got["grad"], want["grad"]),
                                                                                                               name, l2, bound))
    assert not R.train_failures(b, got, want, bnd)
    for seed in (10, 11):
        for rev in (False, True):
            fails = R.train_failures(b, R.emulated_train(b, nudge=np.random.RandomState(seed), rev=rev), want, bnd)
            assert not fails, (seed, rev, fails)


# the assertion that must reject each fault model at trained weights
REJECTED_BY = {"no_hidden_bias": "mu", "no_head_bias": "mu", "tanh_clamped": "mu", "ratio_exp_clamped": "pg_loss", "dy_bf16": "grad L2 pi_fc0/w",
               "last_row_dropped": "grad L2 pi_fc1/w", "clip_pass_dropped": "grad L2 pi/w"}


def failures(b, want, bnd, fault):
    return [f.split(":")[0] for f in R.act_failures(b, R.emulated_act(b, fault), bnd) + R.train_failures(b, R.emulated_train(b, fault), want, bnd)]


@pytest.mark.parametrize("hidden,O,A,n", [((64, 64), 18, 18, 33), ((16, 8, 8), 18, 18, 17), ((256, 256), 18, 18, 40)])
def test_fault_table(hidden, O, A, n):
    assert set(REJECTED_BY) == set(R.FAULTS + R.L2_FAULTS + R.REPLACED_FAULTS)
    b, want, bnd = case(hidden, O, A, n, "trained")
    c, cwant, cbnd = case(hidden, O, A, n, "orth")
    assert not failures(b, want, bnd, None) and not failures(c, cwant, cbnd, None)
    for fault in R.FAULTS + R.L2_FAULTS + R.REPLACED_FAULTS:
        at_trained, at_control = failures(b, want, bnd, fault), failures(c, cwant, cbnd, fault)
        print("%-18s trained: %s\n%-18s control: %s" % (fault, sorted(set(at_trained)), "", sorted(set(at_control))))
        assert REJECTED_BY[fault] in at_trained, (fault, at_trained)
        if fault in R.FAULTS:
            assert not at_control, "the control alone must not notice %s: that is the gap these tests close (%s)" % (fault, at_control)
    # tanh_clamped reaches the value tower too; dy_bf16 is the per-tensor L2 rule's at both weight sets
    assert "value" in failures(b, want, bnd, "tanh_clamped")
    assert "grad L2 pi_fc0/w" in failures(c, cwant, cbnd, "dy_bf16") and "grad L2 pi_fc1/w" in failures(c, cwant, cbnd, "dy_bf16")
    # why clip_pass_dropped was replaced: the control rejects it as well
    assert "grad L2 pi/w" in failures(c, cwant, cbnd, "clip_pass_dropped")


@pytest.mark.parametrize("hidden,n", sorted(R.MEASURED))
def test_measured_guard(hidden, n):
    """the emulation's figures stay within twice the recorded ones, so the bounds cannot rot"""
    _, _, bnd = case(hidden, 18, 18, n, "trained")
    m = bnd["measured"]
    now = dict(mu=m["mu"], v=m["v"], nlp=m["nlp"], loss=float(m["loss"].max()), l2=max(m["l2"].values()), rule=m["rule"])
    print(hidden, n, {k: "%.3g" % x for k, x in now.items()}, "largest L2 at", max(m["l2"], key=m["l2"].get))
    for k, rec in R.MEASURED[(hidden, n)].items():
        assert now[k] <= 2.0 * rec, (k, now[k], rec)


# =====================================================================================================================================================
# GPU
# =====================================================================================================================================================
gpu = pytest.mark.gpu
ACT_SWITCHES = ("PPO_HIP_NO_NARROW",)


def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def handle(b):
    import ppo_cpp_amd
    g = ppo_cpp_amd.PPOHip(b.orc.O, b.orc.A, list(b.orc.hidden))
    g.set_flat(b.theta)
    return g


def delta(before, after):
    return {k: int(after[k] - before.get(k, 0)) for k in after if after[k] != before.get(k, 0)}


def act_figures(b, got):
    err = lambda k, w: float(np.abs(np.asarray(got[k], np.float64) - w).max()) if k in got else float("nan")
    return "mu %.3g action %.3g value %.3g neglogp (sampled) %.3g (given) %.3g" % (err("mu", b.mu), err("action", b.a64), err("value_step", b.v), err("nlp_step", b.nlp_sample),
                                                                                  err("nlp_eval", b.nlp_given))


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,hidden,O,A,n,env,kernel", ACT_CASES, ids=[c[0] for c in ACT_CASES])
def test_act_kernels(name, hidden, O, A, n, env, kernel, kind, monkeypatch):
    need_gpu()
    for s in ACT_SWITCHES:
        monkeypatch.setenv(s, "1" if s in env else "0")
    b, _, bnd = case(hidden, O, A, n, kind)
    g = handle(b)
    try:
        before = g.kernel_counts()
        a, v, nlp = g.step(b.obs, b.noise)
        got = dict(action=a, value_step=v, nlp_step=nlp, value=g.value(b.obs), mu=g.act_deterministic(b.obs))
        got["value_eval"], got["nlp_eval"], got["ent"] = g.evaluate_actions(b.obs, b.actions)
        ran = delta(before, g.kernel_counts())
    finally:
        g.close()
    print("act %s %s: %s; allowances mu %.3g value %.3g neglogp %.3g" % (name, kind, act_figures(b, got), bnd["mu"], bnd["v"], bnd["nlp"]))
    fails = R.act_failures(b, got, bnd)
    assert not fails, fails
    assert ran == {kernel: 3}, ran


def norm_stats(O):
    """non-trivial statistics for the seeded env's U(-1, 1) observations: most columns spread to about +-3, every sixteenth so narrow that it sits at the clip"""
    rng = np.random.RandomState(77)
    mean = rng.uniform(-0.3, 0.3, O).astype(np.float32)
    var = rng.uniform(0.05, 0.3, O).astype(np.float32)
    var[5::16] = 1e-4
    return mean, var, 1e4


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ROLLOUT_CASES)
def test_rollout_kernels(name, kind, monkeypatch):
    need_gpu()
    import ppo_cpp_amd
    from tests import test_rollout_forms as F
    c = F.CASES[name]
    want_ran = json.load(open(F.GOLDEN))["cases"][name]
    F.set_switches(c, monkeypatch.setenv, lambda s: monkeypatch.delenv(s, raising=False))
    E, O, A, T = c["E"], c["O"], 18, F.T
    orc = R.oracle_for(c["hidden"], O, A)
    theta = R.trained_theta(orc, 3) if kind == "trained" else R.orth_theta(orc, 3)
    noise = np.random.RandomState(21).normal(size=(T, E, A)).astype(np.float32)
    g = ppo_cpp_amd.PPOHip(O, A, list(c["hidden"]))
    try:
        g.set_flat(theta)
        g.norm_init(E); g.rollout_alloc(E, T); g.seed(99)
        g.set_norm_stats(0, *norm_stats(O))
        before = g.kernel_counts()
        g.collect_synthetic(1234, GAMMA, LAM, noise, env0=0, step0=0, first=True)
        ran = delta(before, g.kernel_counts())
        obs, a, v, nlp = [g.rollout_get(f) for f in ("obs", "actions", "values", "neglogp")]
    finally:
        g.close()
    assert np.isfinite(obs).all() and np.abs(obs).max() == 10.0 and (np.abs(obs) < 10.0).mean() > 0.8, "the statistics put some, not all, observations at the clip"
    b = R.ActRows(orc, theta, obs.reshape(T * E, O), noise.reshape(T * E, A))
    bnd = R.act_bounds(b)
    got = dict(action=a.reshape(T * E, A), value_step=v.reshape(-1), nlp_step=nlp.reshape(-1))
    print("rollout %s %s: %s; allowances mu %.3g value %.3g neglogp %.3g; max |mu| %.2f" % (name, kind, act_figures(b, got), bnd["mu"], bnd["v"], bnd["nlp"], np.abs(b.mu).max()))
    fails = R.act_failures(b, got, bnd)
    assert not fails, fails
    assert ran == want_ran, (ran, want_ran)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,hidden,O,A,n,env,want_ran", TRAIN_CASES, ids=[c[0] for c in TRAIN_CASES])
def test_train_kernels(name, hidden, O, A, n, env, want_ran, kind, monkeypatch):
    need_gpu()
    from tests import test_train_forms as F
    F.set_switches(dict(env=env), monkeypatch.setenv, lambda s: monkeypatch.delenv(s, raising=False))
    for s in ACT_SWITCHES:
        monkeypatch.setenv(s, "1" if s in env else "0")
    b, want, bnd = case(hidden, O, A, n, kind)
    g = handle(b)
    try:
        before = g.kernel_counts()
        losses = g.train_step(LR, CR, *b.train_args())
        ran = delta(before, g.kernel_counts())
        grad, norm = g.last_grad()
        got = dict(losses=losses, grad=grad, norm=norm, theta=g.get_flat(0), m=g.get_flat(1), v=g.get_flat(2))
    finally:
        g.close()
    tensor, l2, bound = R.l2_report(b, got, want, bnd)
    print("train %s %s: losses off by %s (allowed %s); nearest L2 bound: %s %.3g (bound %.3g, emulation %.3g); the elementwise rule alone: %.2f (emulation %.2f); norm %.3g" % (
        name, kind, np.array2string(np.abs(losses[:4] - want["losses"][:4]), precision=2), np.array2string(np.maximum(1e-6 + 1e-4 * np.abs(want["losses"][:4]), bnd["loss"]), precision=2),
        tensor, l2, bound, bnd["measured"]["l2"][tensor], R.usual_rule_ratio(grad, want["grad"]), bnd["measured"]["rule"], abs(norm - want["norm"]) / want["norm"]))
    fails = R.train_failures(b, got, want, bnd)
    assert not fails, fails
    assert ran == want_ran, (ran, want_ran)
