"""EnvNormalize::step / RunningStatistics::update at trained statistics, in every kernel that restates them, against the float64 model of tests/envnorm_ref.py
(which says what the cases, the emulation, the bounds and the fault models are).

CPU: the emulation at float64 is the model; at float32, in every summation order, it passes every assertion of the GPU tests on every case, and so does the C
oracle's Normalizer; each fault model is rejected by its named case with a margin of 10 bounds; the faults the usual regime hides pass the `fresh` control.
GPU: one handle per (form, case), six env steps as two rollouts of three (the API forms: six calls and a frozen one).  The rollout forms are set up as the
same-named entries of tests/test_rollout_forms.py and must enqueue exactly the kernels tests/golden/rollout_forms.json names for them; set_norm_stats comes
before rollout_reset / the first collect.  Compared: every normalised observation and reward, both statistics after each rollout, the counts exactly."""
import json

import numpy as np
import pytest

from tests import envnorm_ref as R
from tests import test_rollout_forms as F

# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------------
API_FORMS = {"api_e7": (7, 18), "api_e300": (300, 18), "api_cgroups_e300_o64": (300, 64)}      # one chunk | three chunks (one reward chunk) | three splits of 100
DEV_FORMS = ("dev_e1", "dev_e1_no_rollout1", "dev_e8", "dev_e40", "dev_e8_no_persistent", "dev_e96", "dev_o80_e8")
HOST_FORMS = ("host_e1", "host_e8", "host_e40", "host_e8_no_resident", "host_e8_no_fused", "host_256_e16", "host_fused_cat_e8")
# the discrete resident forms: (side, (observations, categories, hidden), environments); (64, 40): nw_nb_rows_per_chunk deals two chunks of 32 rows
RESIDENT_FORMS = {"resident_dev_e8": ("dev", (18, 6, (64, 64)), 8), "resident_host_e8": ("host", (18, 6, (64, 64)), 8),
                  "resident_host_e64_o40": ("host", (40, 6, (32, 32)), 64)}
RESIDENT_SEED = 5                                                       # tests/test_narrow_resident_discrete.SEED

CPU_SHAPES = ([("api", "rows", E, O) for E, O in API_FORMS.values()] + [("rollout", "rows", E, O) for E, O in ((1, 18), (8, 18), (16, 18), (40, 18), (64, 40))] +
              [("rollout", "env", E, O) for E, O in ((1, 18), (8, 18), (40, 18), (96, 18), (8, 80))])


def cases_of(source):
    return R.CASES if source == "rows" else R.DEVICE_CASES


def fmt(d):
    return " ".join("%s %.3g" % (k, v) for k, v in d.items())


# =====================================================================================================================================================
# CPU
# =====================================================================================================================================================
def test_tables_are_consistent():
    assert R.FACTOR == 10.0 and R.MARGIN == 10.0
    from tests import bf16_ref, head_edges_ref
    assert R.FACTOR == head_edges_ref.PART2_FACTOR == bf16_ref.RATE_FACTOR
    assert set(R.REJECTED_BY) == set(R.FAULTS) and set(R.REJECTED_BY.values()) <= set(R.CASES) and set(R.DEVICE_CASES) <= set(R.CASES)
    assert R.T == F.T and R.STEPS == 2 * R.T
    for name in DEV_FORMS + HOST_FORMS:
        assert name in F.ALL_CASES and F.ALL_CASES[name]["side"] == name.split("_")[0], name
    # no environment count used below is a multiple of the float32 spacing at 2^30
    for E in [e for e, _ in API_FORMS.values()] + [F.ALL_CASES[n]["E"] for n in DEV_FORMS + HOST_FORMS] + [e for _, _, e in RESIDENT_FORMS.values()]:
        assert E % 128 != 0
    assert float(np.spacing(np.float32(2.0 ** 30))) == 128.0
    # the chunk deals the shapes are chosen for
    assert R.rows_per_chunk(7, 18) == 7 and R.rows_per_chunk(300, 18) == 100 and R.rows_per_reward_chunk(300) == 320 and R.rows_per_split(300) == 100
    assert R.rows_per_chunk(64, 40) == 32 and R.rows_per_chunk(8, 18) == 8


def test_the_models_outputs_are_finite_on_every_case():
    for mode, source, E, O in CPU_SHAPES:
        for name in cases_of(source):
            case = R.make_case(name, E, O, source)
            for flags in ((True, True), (False, True), (True, False), (False, False)):
                out = R.run(R.Model(case, *flags), case, mode)
                assert all(np.isfinite(v).all() for v in out.values()), (name, mode, E, O, flags)


def test_model_clips_flags_and_frozen_path():
    """the model itself, on what can be said without it: the clips are reached and hold, a frozen step and the flags leave the statistics alone, the raw values
    pass through with a flag off, the return is carried, discounted and reset"""
    case = R.make_case("tiny_ret_var", 40, 18)
    out = R.run(R.Model(case), case, "api")
    assert np.abs(out["rewards"]).max() == R.CLIP_REW and (np.abs(out["rewards"]) == R.CLIP_REW).mean() > 0.95
    case = R.make_case("fast_var", 40, 18)
    out = R.run(R.Model(case), case, "api")
    assert np.abs(out["obs"]).max() <= R.CLIP_OBS
    for key in ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count"):
        np.testing.assert_array_equal(out[key][1], out[key][2], err_msg="the frozen step moved " + key)
    off = R.run(R.Model(case, False, False), case, "api")
    np.testing.assert_array_equal(off["obs"], np.array([s[0] for s in case.steps], np.float64))
    np.testing.assert_array_equal(off["rewards"], np.array([s[1] for s in case.steps], np.float64))
    np.testing.assert_array_equal(off["obs_count"], case.obs0[2]); np.testing.assert_array_equal(off["ret_count"], case.ret0[2])
    m = R.Model(case)
    m.reward(np.ones(40), np.zeros(40)); m.reward(np.ones(40), (np.arange(40) < 3).astype(np.float64))
    np.testing.assert_allclose(m.ret, np.where(np.arange(40) < 3, 0.0, 1.0 + R.GAMMA), rtol=1e-15)
    # two batches merged one after the other are the statistics of their union (Chan)
    rng = np.random.RandomState(3)
    a, b = rng.normal(3.0, 2.0, (50, 4)), rng.normal(-1.0, 0.5, (30, 4))
    mean, var, cnt = R.Model.update(a.mean(0), a.var(0), 50.0, b)
    ab = np.concatenate([a, b])
    np.testing.assert_allclose(mean, ab.mean(0), rtol=1e-13); np.testing.assert_allclose(var, ab.var(0), rtol=1e-13); assert cnt == 80.0


def test_emulation_at_float64_is_the_model():
    worst = 0.0
    for mode, source, E, O in CPU_SHAPES:
        for name in cases_of(source):
            case = R.make_case(name, E, O, source)
            for flags in ((True, True), (False, True), (True, False)) if (E, O) == (8, 18) else ((True, True),):
                want = R.run(R.Model(case, *flags), case, mode)
                for order in R.ORDERS:
                    got = R.run(R.Emu(case, np.float64, order, norm_obs=flags[0], norm_rew=flags[1]), case, mode)
                    for key in R.TOL:
                        scale = np.abs(want[key]).max()
                        err = np.abs(got[key] - want[key]).max()
                        worst = max(worst, err / scale if scale > 0 else err)
                        assert err <= 1e-12 * scale, (name, mode, E, O, order, key, err, scale)
                    for key in R.COUNTS:
                        np.testing.assert_array_equal(got[key], want[key])
    print("largest |emulate(float64) - model| / largest |model| of the output: %.3g" % worst)


def test_float32_emulation_and_c_oracle_pass_every_assertion():
    """the stand-in for a correct kernel, in every summation order, and the fp32 C restatement the project already owns: both inside the bounds on every case,
    so the bounds can be met"""
    for mode, source, E, O in CPU_SHAPES:
        for name in cases_of(source):
            case = R.make_case(name, E, O, source)
            for order in R.ORDERS:
                R.check(R.run(R.Emu(case, np.float32, order), case, mode), name, E, O, source, mode, "emulate(float32, %s) %s E=%d O=%d" % (order, mode, E, O))
            _, ratios = R.check(R.run(R.COracle(case), case, mode), name, E, O, source, mode, "oracle.Normalizer %s E=%d O=%d" % (mode, E, O))
            print("oracle.Normalizer %-8s %-4s E=%-3d O=%-2d %-12s largest |error| / bound: %s" % (mode, source, E, O, name, fmt(ratios)))


def test_measured_emulation_errors_and_bounds():
    """prints err32 of every shape and column block and holds the MEASURED table of tests/envnorm_ref.py to the largest per case and output"""
    top = {name: dict.fromkeys(R.TOL, 0.0) for name in R.CASES}
    for mode, source, E, O in CPU_SHAPES:
        for name in cases_of(source):
            _, bound, err = R.bounds(name, E, O, source, mode)
            print("%-8s %-4s E=%-3d O=%-2d %-12s err32 per block: %s" % (mode, source, E, O, name, "  ".join("%s [%s]" % (k, ", ".join("%.2g" % e for e in err[k])) for k in R.TOL)))
            for k in R.TOL:
                top[name][k] = max(top[name][k], max(err[k]))
                assert np.isfinite(bound[k]).all() and (bound[k] > 0).all()
    print("MEASURED (largest err32 over the shapes and blocks) -> bound = max(10 x, floor):")
    for name in R.CASES:
        print("    %-13s %s" % (name, "  ".join("%s %.2g" % (k, top[name][k]) for k in R.TOL)))
    for name in R.CASES:
        for k in R.TOL:
            rec, now = R.MEASURED[name][k], top[name][k]
            assert now <= 1.5 * rec + 1e-30 and rec <= 1.5 * now + 1e-30, (name, k, rec, now)


FAULT_SHAPE = ("api", "rows", 300, 18)           # three chunks: the between-chunk term exists


def fault_outcome(fault, name, shape=FAULT_SHAPE):
    """({output: the largest |error| / bound over the three orders}, counts exact in every order) of emulate(float32, fault) on a case"""
    mode, source, E, O = shape
    case = R.make_case(name, E, O, source)
    want, bound, _ = R.bounds(name, E, O, source, mode)
    ratios, counts_ok = dict.fromkeys(R.TOL, 0.0), True
    for order in R.ORDERS:
        r, ok = R.worst(R.run(R.Emu(case, np.float32, order, fault), case, mode), want, bound)
        ratios = {k: max(ratios[k], r[k]) for k in R.TOL}
        counts_ok = counts_ok and ok
    return ratios, counts_ok


@pytest.mark.parametrize("fault", R.FAULTS)
def test_each_fault_is_rejected_by_its_case_with_a_margin(fault):
    assert R.rows_per_chunk(FAULT_SHAPE[2], FAULT_SHAPE[3]) < FAULT_SHAPE[2]
    name = R.REJECTED_BY[fault]
    for shape in (FAULT_SHAPE, ("rollout", "rows", 40, 18)):
        if fault == "no_between_chunk_term" and shape != FAULT_SHAPE:
            continue                                 # one chunk at 40 x 18: the fault has nothing to drop
        ratios, counts_ok = fault_outcome(fault, name, shape)
        print("%-24s on %-13s %s E=%d: largest |error| / bound: %s; counts exact: %s" % (fault, name, shape[0], shape[2], fmt(ratios), counts_ok))
        if fault == "float_count":
            assert not counts_ok, "the exact-count assertion must reject a float32 count at 2^30"
            case = R.make_case(name, shape[2], shape[3], shape[1])
            got = R.run(R.Emu(case, np.float32, "sequential", fault), case, shape[0])
            if shape[2] < 64:                        # a batch of less than half the float32 spacing of 128: it stands still
                np.testing.assert_array_equal(got["obs_count"], 2.0 ** 30); np.testing.assert_array_equal(got["ret_count"], 2.0 ** 30)
        else:
            assert max(ratios.values()) >= R.MARGIN, (fault, name, ratios)


def test_what_the_fresh_control_notices():
    """the gap these tests close: the usual regime (norm_init, U(-1, 1)) accepts four of the faults outright; for the others the test says what it does"""
    for fault in R.FAULTS:
        ratios, counts_ok = fault_outcome(fault, "fresh")
        rejected = max(ratios.values()) > 1.0
        print("%-24s on fresh: largest |error| / bound: %s; counts exact: %s -> %s" % (fault, fmt(ratios), counts_ok, "REJECTED" if rejected else "passes"))
        if fault in R.GAP_FAULTS:
            assert not rejected, (fault, ratios)
        if fault == "float_count":
            # its counts are one float32 rounding off the doubles (so `==` notices a float32 count anywhere); that they stop growing shows at 2^30 only
            case = R.make_case("fresh", FAULT_SHAPE[2], FAULT_SHAPE[3])
            got = R.run(R.Emu(case, np.float32, "sequential", fault), case, "api")
            want = R.bounds("fresh", FAULT_SHAPE[2], FAULT_SHAPE[3], "rows", "api")[0]
            assert np.abs(got["obs_count"] - want["obs_count"]).max() <= np.spacing(np.float32(want["obs_count"].max()))
            assert np.all(np.diff(got["obs_count"][:2]) > 0)
        elif fault in R.GAP_FAULTS:
            assert counts_ok


# =====================================================================================================================================================
# GPU
# =====================================================================================================================================================
gpu = pytest.mark.gpu


def preset(g, case):
    g.set_norm_stats(0, *case.obs0)
    g.set_norm_stats(1, case.ret0[0], case.ret0[1], case.ret0[2])


def device_stats(g):
    (m, v, c), (rm, rv, rc) = g.norm_stats(0), g.norm_stats(1)
    return dict(obs_mean=m, obs_var=v, obs_count=np.float64(c), ret_mean=rm[0], ret_var=rv[0], ret_count=np.float64(rc))


class ApiHandle:
    """norm_obs / norm_reward of a handle behind the three calls of envnorm_ref.run"""

    def __init__(self, g):
        self.g = g

    def obs(self, x, training=True):
        return self.g.norm_obs(x, training)

    def reward(self, r, d, training=True):
        return self.g.norm_reward(r, d, training)

    def stats(self):
        return device_stats(self.g)


def drive_rollouts(g, case, side, explicit_noise=None):
    """two rollouts of T steps -> (kernel_counts() delta of the first, the outputs in envnorm_ref.run's layout)"""
    if side == "host":
        g.rollout_reset(case.reset_raw)
    obs, rews, stats, delta = [], [], [], None
    for it in range(2):
        before = g.kernel_counts()
        if side == "dev":
            g.collect_synthetic(R.ENV_SEED, F.GAMMA, F.LAM, None, env0=0, step0=it * R.T, first=(it == 0))
        else:
            for t in range(R.T):
                g.rollout_act(t, None)
                g.rollout_observe(t, *case.steps[it * R.T + t])
            g.rollout_finish(F.GAMMA, F.LAM)
        if it == 0:
            after = g.kernel_counts()
            delta = {k: int(after[k] - before.get(k, 0)) for k in after if after[k] != before.get(k, 0)}
        obs.append(g.rollout_get("obs")); rews.append(g.rollout_get("rewards")); stats.append(device_stats(g))
    out = {"obs": np.concatenate(obs), "rewards": np.concatenate(rews)}
    for key in stats[0]:
        out[key] = np.array([s[key] for s in stats], np.float64)
    return delta, out


def report(form, name, checked):
    print("%s %s: largest |device - model|: %s; of its bound: %s" % (form, name, fmt(checked[0]), fmt(checked[1])))


@gpu
@pytest.mark.parametrize("name", R.CASES)
@pytest.mark.parametrize("form", sorted(API_FORMS))
def test_api_forms(form, name):
    """norm_batch_kernel's row-chunk form (one chunk; three chunks behind norm_finish / combine_group, the reward job's one behind combine_single_column), its
    column-group form (three splits of 100 rows), and one frozen step through obs_normalize_kernel at the trained state"""
    import ppo_cpp_amd
    E, O = API_FORMS[form]
    case = R.make_case(name, E, O)
    g = ppo_cpp_amd.PPOHip(O, 3, [4, 5])
    try:
        g.init_orthogonal(0)
        g.norm_init(E, gamma=R.GAMMA, clip_obs=R.CLIP_OBS, clip_rew=R.CLIP_REW, eps=R.EPS)
        preset(g, case)
        got = R.run(ApiHandle(g), case, "api")
    finally:
        g.close()
    report(form, name, R.check(got, name, E, O, "rows", "api", form))


@gpu
@pytest.mark.parametrize("form,name", [(f, n) for f in DEV_FORMS + HOST_FORMS for n in (R.DEVICE_CASES if f.startswith("dev") else R.CASES)])
def test_rollout_form_cases(form, name, monkeypatch):
    """the forms of tests/test_rollout_forms.py, set up as there; the device env's run the cases that are an initial state only (it cannot be fed rows)"""
    import ppo_cpp_amd
    c = F.ALL_CASES[form]
    assert not c["noise"] and not c["mask"]
    F.set_switches(c, monkeypatch.setenv, lambda s: monkeypatch.delenv(s, raising=False))
    E, O, source = c["E"], c["O"], "env" if c["side"] == "dev" else "rows"
    case = R.make_case(name, E, O, source)
    g = ppo_cpp_amd.PPOHip(O, 18, list(c["hidden"]), action_dist=c["dist"], nvec=c["nvec"], shape_kernels=c["shape_kernels"])
    try:
        g.init_orthogonal(0)
        if c["host_fused"]:
            g.set_host_step_fused(True)
        if c["masking"]:
            g.set_action_masking(True)
        g.norm_init(E); g.rollout_alloc(E, R.T); g.seed(99)
        preset(g, case)
        delta, got = drive_rollouts(g, case, c["side"])
    finally:
        g.close()
    want = json.load(open(F.GOLDEN))["cases"][form]
    assert delta == want, (form, delta, want)
    report(form, name, R.check(got, name, E, O, source, "rollout", form))


@gpu
@pytest.mark.parametrize("form,name", [(f, n) for f in sorted(RESIDENT_FORMS) for n in (R.DEVICE_CASES if RESIDENT_FORMS[f][0] == "dev" else R.CASES)])
def test_discrete_resident_forms(form, name, monkeypatch):
    """narrow_rollout_kernel<cat>: the batch sums in norm_batch_kernel's tree order (nw_chunk_moments_lds), at 64 x 40 with the in-kernel Chan combine of two chunks.
    Set up as tests/test_narrow_resident_discrete.py does."""
    from tests.test_narrow_host_step import case_seed, make_handle
    side, spec, E = RESIDENT_FORMS[form]
    F.set_switches(F.case(side, spec[2], E), monkeypatch.setenv, lambda s: monkeypatch.delenv(s, raising=False))
    O, source = spec[0], "env" if side == "dev" else "rows"
    case = R.make_case(name, E, O, source)
    g = make_handle(spec, case_seed(spec, E), fused=False)
    try:
        g.set_rollout_resident(True)
        g.norm_init(E); g.rollout_alloc(E, R.T); g.seed(RESIDENT_SEED)
        preset(g, case)
        delta, got = drive_rollouts(g, case, side)
    finally:
        g.close()
    assert delta.get("narrow_rollout<cat>") == 1 and set(delta) <= {"narrow_rollout<cat>", "narrow_step_kernel<cat>"}, (form, delta)
    report(form, name, R.check(got, name, E, O, source, "rollout", form))
