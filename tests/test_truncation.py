"""Value bootstrap at time-limit truncations: ppo_gae_ex, ppo_rollout_mark_truncated, ppo_rollout_finish's truncation form, the ITimeLimit mixin of the
host layer and PPO2::bootstrap_truncated, against tests/truncation_ref.py (float64 NumPy GAE with the rule of include/ppo_hip.h, a float64 value tower).

CPU tests: the entry points are declared and exported, the arbiter checks itself, TimeLimit / VecEnv / EnvNormalize forward the mixin.
GPU tests: ppo_gae_ex, the host-Env rollout in every rollout form, the no-mark identity, errors, two ranks, learning.
Tolerances for returns / values are those of tests/test_hip_parity.py and tests/test_discrete_policy.py::check_rollout (rtol 2e-4, atol 2e-5); the bf16
handle uses tests/test_bf16_path.py's (values rtol 3e-2 atol 3e-2, returns rtol 3e-2 atol 5e-2)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import truncation_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppo_cpp_amd", "host")
GAMMA, LAM = 0.99, 0.95
NEW_KERNELS = ("gae_kernel<trunc>", "gae_long_kernel<trunc>", "tval_scatter_kernel")


def close(a, b, rtol=2e-4, atol=2e-5, msg=""):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=msg)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert "int ppo_gae_ex(ppo_handle* h, const float* rewards, const float* values, const float* dones, const float* last_values," in src
    assert "int ppo_rollout_mark_truncated(ppo_handle* h, int32_t t, int32_t count, const int32_t* env_ids, const float* terminal_raw_obs);" in src
    assert "#define PPO_ABI_VERSION 3" in src
    import ppo_cpp_amd
    lib = ppo_cpp_amd.load_library()
    assert hasattr(lib, "ppo_gae_ex") and hasattr(lib, "ppo_rollout_mark_truncated")
    assert lib.ppo_abi_version() == 3
    assert ppo_cpp_amd.PPOHip.OUTPUT_FIELDS["terminal_values"] == 7 and "terminal_values" not in ppo_cpp_amd.PPOHip.FIELDS


def gae_case(seed, T, E, p_done=0.03):
    rng = np.random.RandomState(seed)
    step_dones, trunc = tr.make_marks(rng, T, E, p_done)
    dones, last_dones = tr.shift_dones(step_dones)
    rewards = rng.uniform(-1, 1, (T, E)).astype(np.float32)
    values = rng.normal(size=(T, E)).astype(np.float32)
    last_values = rng.normal(size=E).astype(np.float32)
    tv = np.where(trunc, rng.normal(size=(T, E)), 0.0).astype(np.float32)
    return rewards, values, dones, last_values, last_dones, tv, trunc


def test_arbiter_without_terminal_values_is_the_oracle_gae():
    from oracle import numpy_port as npp
    for T, E in ((16, 33), (128, 4)):
        rw, va, dn, lv, ld, tv, _ = gae_case(T, T, E)
        want = npp.gae(rw, va, dn, lv, ld, GAMMA, LAM)
        close(tr.gae_truncated(rw, va, dn, lv, ld, np.zeros((T, E)), GAMMA, LAM), want, rtol=1e-5, atol=1e-6)
        assert np.abs(tr.gae_truncated(rw, va, dn, lv, ld, tv, GAMMA, LAM) - want).max() > 1e-2      # ... and the terminal values do matter


def fixed_point_case(seed, T, E, gamma, c=0.7, p_done=0.1):
    """rewards c, every value c / (1 - gamma), arbitrary dones of which EVERY one is a truncation"""
    rng = np.random.RandomState(seed)
    step_dones, _ = tr.make_marks(rng, T, E, p_done)
    dones, last_dones = tr.shift_dones(step_dones)
    fp = c / (1.0 - gamma)
    return np.full((T, E), c), np.full((T, E), fp), dones, np.full(E, fp), last_dones, np.where(step_dones > 0, fp, 0.0), fp


def test_arbiter_fixed_point():
    """With V == c / (1 - gamma) everywhere and every done bootstrapped, every TD residual is c + gamma V - V = 0: every return equals V, whatever
    lambda and wherever the dones fall.  Without the bootstrap the rows in front of a done are pulled down."""
    for gamma, lam in ((0.99, 0.95), (0.9, 0.5), (0.97, 1.0)):
        rw, va, dn, lv, ld, tv, fp = fixed_point_case(3, 64, 17, gamma)
        got = tr.gae_truncated(rw, va, dn, lv, ld, tv, gamma, lam)
        assert np.abs(got / fp - 1.0).max() <= 1e-12
        without = tr.gae_truncated(rw, va, dn, lv, ld, np.zeros_like(tv), gamma, lam)
        assert np.abs(without / fp - 1.0).max() > 0.5


FORWARDING_PROGRAM = r"""
#include <cstdio>
#include <memory>
#include "env/env_mock.hpp"
#include "env/time_limit.hpp"
#include "env/vec_env.hpp"
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

// done by itself on every `every`-th step; observation = {id, step count since construction}
struct CountingEnv : Env {
    int id, every, n = 0;
    CountingEnv(int i, int e) : id(i), every(e) {}
    std::string get_action_space() override { return Env::SPACE_CONTINOUS; }
    std::string get_observation_space() override { return Env::SPACE_CONTINOUS; }
    int get_action_space_size() override { return 1; }
    int get_observation_space_size() override { return 2; }
    Mat obs() const { Mat m(1, 2); m(0, 0) = (float)id; m(0, 1) = (float)n; return m; }
    Mat reset() override { Mat m = obs(); m(0, 1) = -1.f; return m; }           // (an observation after a reset is recognisable)
    std::vector<Mat> step(const Mat&) override {
        ++n;
        Mat d = Mat::Zero(1, 1);
        if (every > 0 && n % every == 0) d(0, 0) = 1.f;
        return {obs(), Mat::Ones(1, 1), d};
    }
    void render() override {}
    float get_time() override { return 0.f; }
    Mat get_original_obs() override { return obs(); }
    Mat get_original_rew() override { return Mat::Ones(1, 1); }
    void serialize(nlohmann::json&) override {}
    void deserialize(nlohmann::json&) override {}
};

int main() {
    {   // TimeLimit alone: limit 3 over an env that never ends by itself
        TimeLimit tl(std::make_shared<CountingEnv>(7, 0), 3);
        const Mat a = Mat::Zero(1, 1);
        tl.reset();
        for (int s = 1; s <= 7; ++s) {
            std::vector<Mat> r = tl.step(a);
            const bool cut = s % 3 == 0;
            CHECK(r[2](0, 0) == (cut ? 1.f : 0.f));
            CHECK(tl.get_truncated()(0, 0) == (cut ? 1.f : 0.f));
            if (cut) { CHECK(r[0](0, 1) == -1.f); CHECK(tl.get_terminal_obs()(0, 0) == 7.f && tl.get_terminal_obs()(0, 1) == (float)s); }
            else CHECK(r[0](0, 1) == (float)s);
        }
    }
    {   // an inner done before the limit is a termination and restarts the count: inner done every 2 steps, limit 3 -> never truncated
        TimeLimit tl(std::make_shared<CountingEnv>(1, 2), 3);
        const Mat a = Mat::Zero(1, 1);
        for (int s = 1; s <= 8; ++s) {
            std::vector<Mat> r = tl.step(a);
            CHECK(r[2](0, 0) == (s % 2 == 0 ? 1.f : 0.f));
            CHECK(tl.get_truncated()(0, 0) == 0.f);
        }
    }
    {   // VecEnv: env 0 limit 2, env 1 without the mixin (done by itself every 2 steps), env 2 limit 3, env 3 limit 2
        std::vector<std::shared_ptr<Env>> envs;
        envs.push_back(std::make_shared<TimeLimit>(std::make_shared<CountingEnv>(0, 0), 2));
        envs.push_back(std::make_shared<CountingEnv>(1, 2));
        envs.push_back(std::make_shared<TimeLimit>(std::make_shared<CountingEnv>(2, 0), 3));
        envs.push_back(std::make_shared<TimeLimit>(std::make_shared<CountingEnv>(3, 0), 2));
        VecEnv ve(envs, 2);
        ITimeLimit* tl = dynamic_cast<ITimeLimit*>(static_cast<Env*>(&ve));
        CHECK(tl && tl->has_time_limit());
        const int limit[4] = {2, 0, 3, 2};
        const Mat a = Mat::Zero(4, 1);
        for (int s = 1; s <= 7; ++s) {
            std::vector<Mat> r = ve.step(a);
            const Mat tr = tl->get_truncated(), to = tl->get_terminal_obs();
            CHECK(tr.rows() == 4 && tr.cols() == 1 && to.rows() == 4 && to.cols() == 2);
            for (int e = 0; e < 4; ++e) {
                const bool cut = limit[e] && s % limit[e] == 0;
                CHECK(tr(e, 0) == (cut ? 1.f : 0.f));
                CHECK(r[2](e, 0) == ((cut || (e == 1 && s % 2 == 0)) ? 1.f : 0.f));
                if (cut) CHECK(to(e, 0) == (float)e && to(e, 1) == (float)s);          // env order, and the observation the episode ended on
            }
        }
    }
    {   // a VecEnv of environments without the mixin reports none
        std::vector<std::shared_ptr<Env>> envs;
        for (int i = 0; i < 3; ++i) envs.push_back(std::make_shared<CountingEnv>(i, 2));
        VecEnv ve(envs, 1);
        ITimeLimit* tl = dynamic_cast<ITimeLimit*>(static_cast<Env*>(&ve));
        CHECK(tl && !tl->has_time_limit());
        const Mat a = Mat::Zero(3, 1);
        for (int s = 1; s <= 4; ++s) { ve.step(a); for (int e = 0; e < 3; ++e) CHECK(tl->get_truncated()(e, 0) == 0.f); }
        CountingEnv plain(0, 2);
        CHECK(dynamic_cast<ITimeLimit*>(static_cast<Env*>(&plain)) == nullptr);
    }
    std::puts("ok");
    return 0;
}
"""

# EnvNormalize's forwarding needs no GPU either: its normaliser calls are stubbed (the wrapper under test only forwards the mixin)
NORMALIZE_PROGRAM = r"""
#include <cstdio>
#include <memory>
#include "env/env_mock.hpp"
#include "env/env_normalize.hpp"
#include "env/vec_env.hpp"
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)
extern "C" {
int ppo_norm_init(ppo_handle*, int32_t, float, float, float, float) { return 0; }
int ppo_norm_set_flags(ppo_handle*, int, int) { return 0; }
int ppo_norm_obs(ppo_handle*, const float* raw, int32_t n, int, float* out) { for (int i = 0; i < n * 18; ++i) out[i] = 0.5f * raw[i]; return 0; }
int ppo_norm_reward(ppo_handle*, const float* r, const float*, int32_t n, int, float* out) { for (int i = 0; i < n; ++i) out[i] = r[i]; return 0; }
int ppo_norm_reset_returns(ppo_handle*) { return 0; }
int ppo_norm_get_stats(ppo_handle*, int, float*, float*, double*) { return 0; }
int ppo_norm_set_stats(ppo_handle*, int, const float*, const float*, double) { return 0; }
const char* ppo_last_error(const ppo_handle*) { return ""; }
}
int main() {
    std::vector<std::shared_ptr<Env>> envs;
    for (uint32_t i = 0; i < 3; ++i) envs.push_back(std::make_shared<TimeLimit>(std::make_shared<UnitRewardEnv>(1234u, i), (int)i + 2));      // limits 2, 3, 4
    EnvNormalize env{std::unique_ptr<Env>(new VecEnv(envs, 1)), nullptr, true};
    CHECK(env.has_time_limit());
    UnitRewardEnv twin(1234u, 1);                      // env 1's stream, to know the RAW terminal observation
    twin.reset();                                      // (the pool reset every environment once)
    const Mat a = Mat::Zero(3, 18);
    for (int s = 1; s <= 3; ++s) {
        const std::vector<Mat> tw = twin.step(Mat::Zero(1, 18));
        const std::vector<Mat> r = env.step(a);
        const Mat tr = env.get_truncated(), to = env.get_terminal_obs();
        CHECK(tr(0, 0) == (s == 2 ? 1.f : 0.f) && tr(1, 0) == (s == 3 ? 1.f : 0.f) && tr(2, 0) == 0.f);
        CHECK(r[1](1, 0) == 1.f);
        if (s == 3) for (int j = 0; j < 18; ++j) { CHECK(to(1, j) == tw[0](0, j)); CHECK(r[0](1, j) != 0.5f * tw[0](0, j)); }     // raw, not scaled; step() returned the reset observation
    }
    EnvNormalize bare{std::unique_ptr<Env>(new UnitRewardEnv(1234u, 0)), nullptr, true};
    CHECK(!bare.has_time_limit());
    bare.step(Mat::Zero(1, 18));
    CHECK(bare.get_truncated()(0, 0) == 0.f);
    std::puts("ok");
    return 0;
}
"""


def _compile_and_run(tmp_path, src, name):
    cpp = tmp_path / (name + ".cpp")
    cpp.write_text(src)
    exe = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-I", HOST, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(cpp)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)


def test_time_limit_and_vecenv_forward_the_mixin(tmp_path):
    r = _compile_and_run(tmp_path, FORWARDING_PROGRAM, "tl_forwarding")
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_env_normalize_forwards_the_raw_terminal_observation(tmp_path):
    r = _compile_and_run(tmp_path, NORMALIZE_PROGRAM, "tl_normalize")
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


# ---- GPU: ppo_gae_ex ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("T,E,kernel", [(16, 4096, "gae_kernel<trunc>"), (2048, 1, "gae_long_kernel<trunc>"), (128, 64, "gae_long_kernel<trunc>")])
def test_gae_ex_matches_the_arbiter(T, E, kernel):
    import ppo_cpp_amd
    g = ppo_cpp_amd.PPOHip(18, 18, [64, 64])
    rw, va, dn, lv, ld, tv, trunc = gae_case(T + E, T, E)
    assert trunc[0, 0] and trunc[T - 1, 0] and ld[0] == 1.0
    print("T=%d E=%d: %d dones, %d truncated" % (T, E, int(dn.sum() + ld.sum()), int(trunc.sum())))
    before = g.kernel_counts()
    got = g.gae(rw, va, dn, lv, ld, GAMMA, LAM, terminal_values=tv)
    want = tr.gae_truncated(rw, va, dn, lv, ld, tv, GAMMA, LAM)
    print("max abs error %.3g" % np.abs(got - want).max())
    close(got, want, msg="returns")
    after = g.kernel_counts()
    ran = {k: after.get(k, 0) - before.get(k, 0) for k in NEW_KERNELS[:2]}
    assert ran == {k: int(k == kernel) for k in NEW_KERNELS[:2]}, ran
    # NULL terminal values: ppo_gae itself, bit for bit, and not the new kernels
    plain = g.gae(rw, va, dn, lv, ld, GAMMA, LAM)
    np.testing.assert_array_equal(plain, g.gae(rw, va, dn, lv, ld, GAMMA, LAM, terminal_values=None))
    np.testing.assert_array_equal(plain, g.gae(rw, va, dn, lv, ld, GAMMA, LAM, terminal_values=np.zeros((T, E), np.float32)))
    assert np.abs(plain - want).max() > 1e-2
    assert g.kernel_counts().get(kernel) == after[kernel] + 1
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("T,E", [(64, 300), (512, 8)])
def test_gae_ex_fixed_point_in_fp32(T, E):
    import ppo_cpp_amd
    g = ppo_cpp_amd.PPOHip(18, 18, [64, 64])
    for gamma, lam in ((0.99, 0.95), (0.9, 0.5)):
        rw, va, dn, lv, ld, tv, fp = fixed_point_case(T, T, E, gamma)
        got = g.gae(rw, va, dn, lv, ld, gamma, lam, terminal_values=tv)
        print("gamma %.2f: max relative deviation from %.4f: %.3g" % (gamma, fp, np.abs(got / fp - 1).max()))
        np.testing.assert_allclose(got, fp, rtol=1e-5)
        assert np.abs(g.gae(rw, va, dn, lv, ld, gamma, lam) / fp - 1).max() > 0.5
    g.close()


# ---- GPU: the host-Env rollout in every rollout form -----------------------------------------------------------------------------------
def make_handle(O, A, hidden, seed, dist="gaussian", bf16=False):
    import ppo_cpp_amd
    g = ppo_cpp_amd.PPOHip(O, A, list(hidden), action_dist=dist, **({"compute_dtype": 1} if bf16 else {}))
    g.init_orthogonal(seed)
    # a value head far from zero and biases that matter (the orthogonal initialiser leaves the biases at 0)
    rng = np.random.RandomState(seed)
    theta = g.get_flat(0)
    g.set_flat((theta + rng.uniform(-0.05, 0.05, theta.size)).astype(np.float32))
    return g


def ran(g):
    """the kernel variants enqueued so far (kernel_counts lists every variant, most of them at 0)"""
    return {k: v for k, v in g.kernel_counts().items() if v}


def rollout_case(seed, T, E, O, p_done=0.03):
    rng = np.random.RandomState(seed)
    step_dones, trunc = tr.make_marks(rng, T, E, p_done)
    term_raw = rng.uniform(-1.5, 1.5, (T, E, O)).astype(np.float32)
    return step_dones, trunc, term_raw


FORMS = [  # id, hidden, E, T, dist, bf16, explicit noise, the kernel that must serve the rollout's act steps
    ("resident1", (64, 64), 1, 64, "gaussian", False, False, "narrow_rollout1_kernel"),
    ("resident64", (64, 64), 64, 16, "gaussian", False, False, "narrow_rollout_kernel"),
    ("fused32", (64, 64), 32, 16, "gaussian", False, True, None),
    ("steps256", (64, 64), 256, 8, "gaussian", False, True, "narrow_step_kernel<static>"),
    ("wide256", (256, 256), 256, 8, "gaussian", False, True, "policy_step_kernel"),
    ("bf16", (256, 256), 256, 8, "gaussian", True, True, "bf16_step_sequence"),
    ("categorical", (64, 64), 256, 8, "categorical", False, True, "policy_step_kernel<cat>"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_host_env_rollout_matches_the_arbiter(form):
    _, hidden, E, T, dist, bf16, explicit, kernel = form
    O, A, seed = 18, 18 if dist == "gaussian" else 7, 321
    step_dones, trunc, term_raw = rollout_case(E + T, T, E, O, p_done=0.03 if E * T > 256 else 0.1)
    K = int(trunc.sum())
    assert trunc[0, 0] and trunc[T - 1, 0] and K >= 2
    rng = np.random.RandomState(2)
    noise = (rng.normal(size=(T, E, A)) if dist == "gaussian" else rng.uniform(size=(T, E, A))).astype(np.float32) if explicit else None
    runs = {}
    for mark in (True, False):
        g = make_handle(O, A, hidden, 9, dist, bf16)
        g.seed(77)
        g.norm_init(E)
        g.rollout_alloc(E, T)
        tr.host_rollout(g, seed, E, T, step_dones, trunc, term_raw, GAMMA, LAM, noise, mark=mark)
        runs[mark] = dict(returns=g.rollout_get("returns"), values=g.rollout_get("values"), tv=g.rollout_get("terminal_values"), obs=g.rollout_get("obs"),
                          rewards=g.rollout_get("rewards"), dones=g.rollout_get("dones"), rms=g.norm_stats(0), ret_rms=g.norm_stats(1), kc=ran(g))
        if mark:
            ref = tr.ref_rollout(g, seed, E, T, step_dones, trunc, term_raw, GAMMA, LAM)
        g.close()
    got, plain = runs[True], runs[False]
    vt = dict(rtol=3e-2, atol=3e-2) if bf16 else dict(rtol=2e-4, atol=2e-5)
    rt = dict(rtol=3e-2, atol=5e-2) if bf16 else dict(rtol=2e-4, atol=2e-5)
    close(got["obs"], ref["obs"], rtol=2e-4, atol=2e-5, msg="obs")
    close(got["rewards"], ref["rewards"], msg="rewards")
    np.testing.assert_array_equal(got["dones"], ref["dones"])
    close(got["values"], ref["values"], msg="values", **vt)
    print("%s: K=%d  max |tv - ref| %.3g  max |returns - ref| %.3g  max |tv| %.3g" % (form[0], K, np.abs(got["tv"] - ref["terminal_values"]).max(),
                                                                                  np.abs(got["returns"] - ref["returns"]).max(), np.abs(ref["terminal_values"]).max()))
    # terminal values: the arbiter's V(normalise_at_finish(raw terminal obs)) on the marked rows, EXACTLY 0 elsewhere
    close(got["tv"][trunc], ref["terminal_values"][trunc], msg="terminal values", **vt)
    assert np.all(got["tv"][~trunc] == 0.0)
    assert np.abs(ref["terminal_values"][trunc]).min() > 1e-3
    close(got["returns"], ref["returns"], msg="returns", **rt)
    assert np.abs(plain["returns"] - ref["returns"]).max() > 10 * rt["atol"]                   # (the marks matter at this tolerance)
    assert np.all(plain["tv"] == 0.0)
    # the terminal observations never enter the statistics, and the reward normaliser does not see the bootstrap
    for a, b in zip(got["rms"] + got["ret_rms"], plain["rms"] + plain["ret_rms"]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(got["values"], plain["values"])
    np.testing.assert_array_equal(got["rewards"], plain["rewards"])
    # kernels: the truncation form of GAE and the scatter ran once; the marks cost ONE more value pass; the rollout form itself is the unmarked run's
    kc, kp = got["kc"], plain["kc"]
    long_form = E <= 64 and T >= 128
    assert kc.get("gae_long_kernel<trunc>", 0) == int(long_form) and kc.get("gae_kernel<trunc>", 0) == int(not long_form) and kc["tval_scatter_kernel"] == 1
    assert not any(k in kp for k in NEW_KERNELS)
    step_name = {"categorical": "policy_step_kernel<cat>"}.get(dist, "bf16_step_sequence" if bf16 else "narrow_step_kernel<static>" if hidden == (64, 64) else "policy_step_kernel")
    rest = {k: v for k, v in kc.items() if k not in NEW_KERNELS}
    want = dict(kp)
    want[step_name] = want.get(step_name, 0) + 1
    assert rest == want, (rest, kp)
    if kernel:
        assert kc.get(kernel, 0) >= 1, kc


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,E,T", [((64, 64), 1, 32), ((64, 64), 64, 8), ((256, 256), 256, 4)])
def test_a_rollout_without_marks_is_untouched(hidden, E, T):
    """Two handles in one process: one never calls the new entry point, one calls it with count = 0 after every observe.  Bitwise the same returns, the same
    kernel_counts dictionary, none of the new kernels."""
    O, A = 18, 18
    step_dones, trunc, term_raw = rollout_case(5, T, E, O, p_done=0.1)
    out = []
    for call in (False, True):
        g = make_handle(O, A, hidden, 4)
        g.seed(5)
        g.norm_init(E)
        g.rollout_alloc(E, T)
        from oracle import oracle as o
        raw, _, _ = o.seeded_env_step(11, 0, E, 0, O)
        g.rollout_reset(raw)
        for t in range(T):
            g.rollout_act(t)
            raw, rew, _ = o.seeded_env_step(11, 0, E, t + 1, O)
            g.rollout_observe(t, raw, rew, step_dones[t])
            if call:
                g.rollout_mark_truncated(t, np.zeros(0, np.int32), np.zeros((0, O), np.float32))
        g.rollout_finish(GAMMA, LAM)
        out.append((g.rollout_get("returns"), g.rollout_get("actions"), ran(g), g.rollout_get("terminal_values")))
        g.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and not any(k in out[0][2] for k in NEW_KERNELS), (out[0][2], out[1][2])
    assert np.all(out[0][3] == 0.0) and np.all(out[1][3] == 0.0)


@pytest.mark.gpu
def test_errors_leave_the_list_alone_and_the_list_does_not_leak():
    import ppo_cpp_amd
    O, A, E, T = 18, 18, 8, 6
    step_dones = np.zeros((T, E), np.float32)
    step_dones[2, 3] = step_dones[2, 5] = step_dones[4, 1] = 1.0
    trunc = step_dones > 0
    term_raw = np.random.RandomState(0).uniform(-1, 1, (T, E, O)).astype(np.float32)
    from oracle import oracle as o

    def run(g, marks, bad_calls):
        raw, _, _ = o.seeded_env_step(3, 0, E, 0, O)
        g.rollout_reset(raw)
        for t in range(T):
            g.rollout_act(t)
            raw, rew, _ = o.seeded_env_step(3, 0, E, t + 1, O)
            g.rollout_observe(t, raw, rew, step_dones[t])
            if bad_calls and t == 2:
                for args, what in (((2, [8], term_raw[2, :1]), "out of range"), ((2, [-1], term_raw[2, :1]), "out of range"),
                                   ((2, [0], term_raw[2, :1]), "done is 0"), ((2, [3, 0], term_raw[2, :2]), "done is 0"),
                                   ((2, [3, 3], term_raw[2, :2]), "twice"), ((T, [3], term_raw[2, :1]), "bad step"),
                                   ((-1, [3], term_raw[2, :1]), "bad step"), ((1, [3], term_raw[2, :1]), "last ppo_rollout_observe")):
                    with pytest.raises(ppo_cpp_amd.PPOHipError, match=what):
                        g.rollout_mark_truncated(*args)
                assert g.lib.ppo_rollout_mark_truncated(g.h, 2, -1, None, None) != 0
            ids = np.nonzero(trunc[t])[0]
            if marks and ids.size:
                g.rollout_mark_truncated(t, ids[:1], term_raw[t, ids[:1]])         # in two calls: the list appends
                if ids.size > 1:
                    g.rollout_mark_truncated(t, ids[1:], term_raw[t, ids[1:]])
                if bad_calls:
                    with pytest.raises(ppo_cpp_amd.PPOHipError, match="already marked"):
                        g.rollout_mark_truncated(t, ids[:1], term_raw[t, ids[:1]])
        g.rollout_finish(GAMMA, LAM)
        return g.rollout_get("returns"), g.rollout_get("terminal_values")

    def fresh():
        g = make_handle(O, A, (64, 64), 2)
        g.seed(1)
        return g

    g = fresh()
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="ppo_rollout_alloc"):
        g.rollout_mark_truncated(0, [0], term_raw[0, :1])
    g.norm_init(E)
    g.rollout_alloc(E, T)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="output"):
        g.rollout_set("terminal_values", np.zeros((T, E), np.float32))
    ret_bad, tv_bad = run(g, True, True)                  # every error in the middle of a correct marked rollout
    ret2, tv2 = run(g, False, False)                      # the SAME handle, a second rollout without marks
    g.close()
    g = fresh(); g.norm_init(E); g.rollout_alloc(E, T)
    ret_good, tv_good = run(g, True, False)               # a marked rollout without the failed calls
    ret2_ref, tv2_ref = run(g, False, False)
    g.close()
    np.testing.assert_array_equal(ret_bad, ret_good)
    np.testing.assert_array_equal(tv_bad, tv_good)
    assert (tv_good != 0).sum() == 3
    g = fresh(); g.norm_init(E); g.rollout_alloc(E, T)
    run(g, False, False)                                  # never a mark on this handle
    ret2_plain, _ = run(g, False, False)
    g.close()
    # rollout 2 equals an unmarked run bitwise: same statistics history (the marks never touch it), no terminal value left over
    np.testing.assert_array_equal(ret2, ret2_ref)
    np.testing.assert_array_equal(ret2, ret2_plain)
    assert np.all(tv2 == 0.0) and np.all(tv2_ref == 0.0)
    # a mark that is followed by a reset is forgotten
    g = fresh(); g.norm_init(E); g.rollout_alloc(E, T)
    raw, rew, _ = o.seeded_env_step(3, 0, E, 1, O)
    g.rollout_reset(raw); g.rollout_act(0); g.rollout_observe(0, raw, rew, np.ones(E, np.float32))
    g.rollout_mark_truncated(0, [0, 1], term_raw[0, :2])
    ret_a, tv_a = run(g, False, False)
    assert np.all(tv_a == 0.0)
    g.close()


# ---- GPU: two ranks ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_ranks_mark_their_own_environments(tmp_path):
    """world 2 on the collective-library stand-in (two processes on one GPU, tests/fake_rccl): every rank runs the host-Env loop over its half of the
    environments and marks its own truncations; the observation statistics are the job's.  Each rank's returns match the arbiter over the union, and
    the replicas are bit-identical after an update."""
    from tests.test_dp_two_ranks import build_fake_rccl
    world, hidden, E, T, O, A = 2, (64, 64), 32, 16, 18, 18
    tmp = str(tmp_path)
    fake = build_fake_rccl(tmp)
    step_dones, trunc, term_raw = rollout_case(12, T, E, O, p_done=0.06)
    trunc[3, E - 1] = True; step_dones[3, E - 1] = 1.0             # (both ranks have marks)
    g = make_handle(O, A, hidden, 6)
    theta = g.get_flat(0)
    ref = tr.ref_rollout(g, 55, E, T, step_dones, trunc, term_raw, GAMMA, LAM)
    g.close()
    uid = np.zeros(128, np.uint8)
    name = ("/ppo_dp_trunc_%d" % os.getpid()).encode()
    uid[:len(name)] = np.frombuffer(name, np.uint8)
    fin = os.path.join(tmp, "in.npz")
    np.savez(fin, hidden=np.array(hidden), E=E, T=T, O=O, A=A, theta=theta, uid=uid, step_dones=step_dones, trunc=trunc, term_raw=term_raw, seed=55,
             gamma=GAMMA, lam=LAM)
    env = dict(os.environ, PPO_RCCL_LIBRARY=fake, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dp_worker_truncation.py"), str(r), str(world), fin, os.path.join(tmp, "out%d.npz" % r)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=300)[0].decode())
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("data-parallel workers timed out")
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    outs = [np.load(os.path.join(tmp, "out%d.npz" % r)) for r in range(world)]
    El = E // world
    for r, out in enumerate(outs):
        sl = slice(r * El, (r + 1) * El)
        assert trunc[:, sl].sum() >= 1
        close(out["values"], ref["values"][:, sl], msg="values rank %d" % r)
        close(out["tv"][trunc[:, sl]], ref["terminal_values"][:, sl][trunc[:, sl]], msg="terminal values rank %d" % r)
        assert np.all(out["tv"][~trunc[:, sl]] == 0.0)
        close(out["returns"], ref["returns"][:, sl], msg="returns rank %d" % r)
        assert int(out["scatter"]) == 1
    for k in ("theta", "adam_m", "adam_v", "obs_mean", "obs_var"):
        np.testing.assert_array_equal(outs[0][k], outs[1][k])
    assert np.abs(outs[0]["theta"] - theta).max() > 0


# ---- GPU: learning -------------------------------------------------------------------------------------------------------------
BAND, MID = 0.032, 8.156


@pytest.mark.gpu
def test_ppo2_learns_the_value_of_a_time_limited_task():
    """Learning: 16 x TimeLimit(UnitRewardEnv, 20) (host/env/env_mock.hpp: reward 1 on every step, episodes end by the time limit only) behind VecEnv +
    EnvNormalize (norm_reward off), gamma 0.9, lambda 0.95, 32 steps, [64,64], 60 updates of 4 epochs x 4 minibatches at lr 1e-3, cliprange 0.2, through
    PPO2::learn with the library's own sampling and shuffles.  With the bootstrap every TD residual of a position-blind critic c is 1 + gamma c - c, at the
    truncations and at the rollout's end alike: its fixed point is 1 / (1 - gamma) = 10 whatever lambda is.  Without it the critic settles near the mean of
    the truncated sums, about 6.  The figure is the mean V over a fixed probe batch (64 observations the environments visit: truncation_ref.probe_batch).
    The arbiter's NumPy loop (truncation_ref.learn_unit_reward, the oracle's policy and update) over seeds 1, 2, 3 after 60 updates:
      bootstrapped   10.004, 10.001, 10.017  (mean 10.007, spread 0.016)        not bootstrapped   6.328, 6.305, 6.281  (mean 6.305)
    (a) bootstrapped run: |mean V - 10| <= BAND = 0.032, twice the arbiter's seed spread.  (b) the run of the same seed with bootstrap_truncated off ends
    below MID = 8.156, the midpoint between the arbiter's two means.
    This leg on an MI355X (seed 3): bootstrapped 10.008, not bootstrapped 6.315."""
    from ppo_cpp_amd import hostapi
    probe = tr.probe_batch()
    kw = dict(n_envs=16, n_steps=32, hidden=[64, 64], n_updates=60, nminibatches=4, noptepochs=4, lr=1e-3, cliprange=0.2, time_limit=20, probe_raw=probe,
              gamma=0.9, lam=0.95, seed=3, norm_obs=True, norm_reward=False)
    boot = hostapi.learn_time_limit(bootstrap_truncated=True, **kw)["probe_values"].mean()
    plain = hostapi.learn_time_limit(bootstrap_truncated=False, **kw)["probe_values"].mean()
    print("mean V over the probe batch: bootstrapped %.3f, not bootstrapped %.3f" % (boot, plain))
    assert abs(boot - 10.0) <= BAND, (boot, BAND)
    assert plain < MID, (plain, MID)


