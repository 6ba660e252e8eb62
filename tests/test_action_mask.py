"""Action masks for categorical policies (include/ppo_hip.h, "action masks of the categorical head") against tests/masked_categorical_ref.py
(float64 NumPy forward with the excluded-category formulas, torch float64 autograd of sb3-contrib's masked expressions for the loss).

CPU tests: the entry points are declared and exported, the reference's gradient and masked sampler are right.
GPU tests: step / train step / host-Env rollout / update against the reference, same bits under all-ones masks, kernel selection, errors.
Tolerances and the near-tie rule are those of tests/test_discrete_policy.py; the share of near-tie rows is printed and bounded at 1 %."""
import os
import subprocess

import numpy as np
import pytest

from tests.masked_categorical_ref import MaskedCatRef, masked_gumbel_argmax, masked_softmax_stats, random_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppo_cpp_amd", "host")
CR = 0.16102319955825806
LR = 0.000393141177482903
GAMMA, LAM = 0.99, 0.95
TIE = 1e-5          # a row whose two best perturbed ALLOWED logits are closer than this may go either way in fp32

NEW_SYMBOLS = ("ppo_step_masked", "ppo_act_deterministic_masked", "ppo_train_step_masked", "ppo_set_action_masking", "ppo_get_action_masking",
               "ppo_rollout_act_masked")


def close(a, b, rtol=1e-4, atol=1e-5, msg=""):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=msg)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_masked_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert "%s(" % name in src, name
    assert "#define PPO_ABI_VERSION 3" in src
    import ppo_cpp_amd
    lib = ppo_cpp_amd.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.ppo_abi_version() == 3


def test_reference_gradient_matches_central_differences_with_masks():
    """The autograd arbiter itself: d loss / d theta against central finite differences of the same float64 loss, 12 rows with masks."""
    ref = MaskedCatRef(5, 4, [6, 3], ent_coef=0.05)
    ref.init_random(3)
    rng = np.random.RandomState(0)
    n = 12
    obs = rng.uniform(-1, 1, (n, 5))
    mask = random_masks(rng, n, 4)
    assert (mask == 0).any() and (mask.sum(1) >= 1).all()
    a, v, nlp, _ = ref.step(obs, rng.uniform(size=(n, 4)), mask)
    assert np.all(mask[np.arange(n), a] != 0)
    old_nlp = nlp + rng.normal(scale=0.05, size=n)
    old_v = v + rng.normal(scale=0.05, size=n)
    ret = v + rng.normal(scale=0.5, size=n)
    adv = rng.normal(size=n)
    args = (obs, a, adv, ret, old_nlp, old_v, 0.3, mask)
    losses, grad = ref.loss_grad(*args)
    # the autograd loss values are the closed formulas of the header
    nlp_all, ent, _ = masked_softmax_stats(ref.forward(obs)[0], mask)
    np.testing.assert_allclose(losses[2], ent.mean(), rtol=1e-12)
    np.testing.assert_allclose(losses[3], 0.5 * np.mean((nlp_all[np.arange(n), a] - old_nlp) ** 2), rtol=1e-12)

    def loss_at(theta):
        keep = ref.theta.copy()
        ref.theta[:] = theta
        l5, _ = ref.loss_grad(*args)
        ref.theta[:] = keep
        return l5[0] - ref.ent * l5[2] + ref.vfc * l5[1]

    h = 1e-6
    fd = np.empty(ref.P)
    for i in range(ref.P):
        tp, tm = ref.theta.copy(), ref.theta.copy()
        tp[i] += h; tm[i] -= h
        fd[i] = (loss_at(tp) - loss_at(tm)) / (2 * h)
    np.testing.assert_allclose(grad, fd, rtol=1e-5, atol=1e-8)


def test_reference_masked_sampler_reproduces_renormalised_frequencies():
    rng = np.random.RandomState(1)
    logits = np.array([[1.5, -0.3, 0.2, 0.9, -2.0]])
    mask = np.array([[1.0, 0.0, 1.0, 0.0, 1.0]])
    N = 200000
    a, _ = masked_gumbel_argmax(np.repeat(logits, N, 0), rng.uniform(size=(N, 5)), np.repeat(mask, N, 0))
    _, _, p = masked_softmax_stats(logits, mask)
    assert p[0][1] == 0 and p[0][3] == 0 and abs(p[0].sum() - 1) < 1e-12
    freq = np.bincount(a, minlength=5) / N
    assert freq[1] == 0 and freq[3] == 0                       # never a forbidden category
    sigma = np.sqrt(p[0] * (1 - p[0]) / N)
    assert np.all(np.abs(freq - p[0]) <= 4 * sigma), (freq, p[0])


# MaskedTargetEnv and the IActionMask mixin through VecEnv + EnvNormalize need no GPU: the normaliser calls are stubbed (the wrappers under test only forward the mixin).
# `dump E N file` writes the environments' action-independent stream (raw observations, masks, targets): what the NumPy reference loop behind the thresholds of
# test_ppo2_learns_the_masked_target_task was fed.
HOST_PROGRAM = r"""#include <cstdio>
#include <cstdlib>
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
// argv: dump E N file -> for step 0..N-1 of environments 0..E-1: raw obs [E,18] | mask [E,18] | target [E] (floats); the stream does not depend on the actions
static int dump(int E, int N, const char* path) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return 2;
    std::vector<std::shared_ptr<MaskedTargetEnv>> envs;
    for (int e = 0; e < E; ++e) { envs.push_back(std::make_shared<MaskedTargetEnv>(1234u, (uint32_t)e)); envs.back()->reset(); }
    for (int s = 0; s < N; ++s) {
        for (auto& e : envs) { const Mat o = e->get_original_obs(); std::fwrite(o.data(), sizeof(float), 18, f); }
        for (auto& e : envs) { const Mat m = e->get_action_mask(); std::fwrite(m.data(), sizeof(float), 18, f); }
        for (auto& e : envs) { const float t = (float)e->target(); std::fwrite(&t, sizeof(float), 1, f); }
        Mat a(1, 1);
        for (auto& e : envs) { a(0, 0) = (float)e->target(); e->step(a); }
    }
    std::fclose(f);
    return 0;
}
int main(int argc, char** argv) {
    if (argc == 5 && std::string(argv[1]) == "dump") return dump(std::atoi(argv[2]), std::atoi(argv[3]), argv[4]);
    const int A = 18;
    {   // MaskedTargetEnv alone: the target is always allowed, about half of the others are not, rewards 1 / 0 / -1, forbidden actions are counted
        MaskedTargetEnv env(1234u, 3);
        DiscreteTargetEnv twin(1234u, 3);                 // the same W and observation stream
        CHECK(dynamic_cast<IActionMask*>(static_cast<Env*>(&env)) != nullptr && env.has_action_mask());
        CHECK(dynamic_cast<IActionMask*>(static_cast<Env*>(&twin)) == nullptr);
        Mat o = env.reset(), ot = twin.reset();
        long open = 0, sent_forbidden = 0;
        Mat a(1, 1);
        for (int s = 0; s < 300; ++s) {
            for (int j = 0; j < 18; ++j) CHECK(o(0, j) == ot(0, j));
            const Mat m = env.get_action_mask();
            CHECK(m.rows() == 1 && m.cols() == A);
            const int tgt = env.target();
            CHECK(m(0, tgt) == 1.f);
            int n_open = 0, other = -1, closed = -1;
            for (int j = 0; j < A; ++j) { CHECK(m(0, j) == 0.f || m(0, j) == 1.f); n_open += m(0, j) != 0.f; if (m(0, j) != 0.f && j != tgt) other = j; if (m(0, j) == 0.f) closed = j; }
            open += n_open;
            const Mat m2 = env.get_action_mask();
            for (int j = 0; j < A; ++j) CHECK(m2(0, j) == m(0, j));                 // asking does not move the stream
            const int pick = s % 3 == 0 ? tgt : s % 3 == 1 && other >= 0 ? other : closed >= 0 ? closed : tgt;
            a(0, 0) = (float)pick;
            const std::vector<Mat> r = env.step(a);
            a(0, 0) = (float)tgt;
            const std::vector<Mat> rt = twin.step(a);
            CHECK(rt[1](0, 0) == 1.f);                                                // the twin agrees on the target
            const float want = pick == tgt ? 1.f : m(0, pick) != 0.f ? 0.f : -1.f;
            CHECK(r[1](0, 0) == want && env.get_original_rew()(0, 0) == want);
            sent_forbidden += want == -1.f;
            CHECK(env.forbidden_received() == sent_forbidden);
            CHECK(r[2](0, 0) == ((s + 1) % 100 == 0 ? 1.f : 0.f));
            o = r[0]; ot = rt[0];
        }
        CHECK(sent_forbidden > 50);
        const double share = (double)open / (300.0 * A);
        CHECK(share > 0.45 && share < 0.62);              // half of the 17 others plus the target: about 0.53
    }
    {   // VecEnv: masked children and one without the mixin (all ones), in environment order; then behind EnvNormalize, unscaled
        std::vector<std::shared_ptr<Env>> envs;
        std::vector<std::shared_ptr<MaskedTargetEnv>> twins;
        for (uint32_t i = 0; i < 4; ++i) {
            if (i == 2) { envs.push_back(std::make_shared<DiscreteTargetEnv>(1234u, i)); twins.push_back(nullptr); }
            else { envs.push_back(std::make_shared<MaskedTargetEnv>(1234u, i)); twins.push_back(std::make_shared<MaskedTargetEnv>(1234u, i)); twins.back()->reset(); }
        }
        EnvNormalize env{std::unique_ptr<Env>(new VecEnv(envs, 2)), nullptr, true};
        IActionMask* am = dynamic_cast<IActionMask*>(static_cast<Env*>(&env));
        CHECK(am && am->has_action_mask());
        IActionMask* inner = dynamic_cast<IActionMask*>(&env.inner());
        CHECK(inner && inner->has_action_mask());
        env.reset();
        Mat a = Mat::Zero(4, 1);
        for (int s = 0; s < 5; ++s) {
            const Mat m = am->get_action_mask(), mi = inner->get_action_mask();
            CHECK(m.rows() == 4 && m.cols() == A);
            for (int e = 0; e < 4; ++e) {
                const Mat want = twins[e] ? twins[e]->get_action_mask() : Mat::Ones(1, A);
                for (int j = 0; j < A; ++j) CHECK(m(e, j) == want(0, j) && mi(e, j) == want(0, j));
            }
            env.step(a);
            Mat a1 = Mat::Zero(1, 1);
            for (auto& t : twins) if (t) t->step(a1);
        }
    }
    {   // nothing inside carries the mixin: the containers report false and all ones
        std::vector<std::shared_ptr<Env>> envs;
        for (uint32_t i = 0; i < 3; ++i) envs.push_back(std::make_shared<DiscreteTargetEnv>(1234u, i));
        VecEnv ve(envs, 1);
        CHECK(!ve.has_action_mask());
        const Mat m = ve.get_action_mask();
        for (int e = 0; e < 3; ++e) for (int j = 0; j < A; ++j) CHECK(m(e, j) == 1.f);
        EnvNormalize bare{std::unique_ptr<Env>(new DiscreteTargetEnv(1234u, 0)), nullptr, true};
        CHECK(!bare.has_action_mask());
        CHECK(bare.get_action_mask().cols() == A && bare.get_action_mask()(0, 5) == 1.f);
    }
    std::puts("ok");
    return 0;
}
"""


def test_masked_target_env_and_mixin_forwarding(tmp_path):
    cpp = tmp_path / "mask_host.cpp"
    cpp.write_text(HOST_PROGRAM)
    exe = tmp_path / "mask_host"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-I", HOST, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(cpp)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_host_entry_point_is_exported():
    from ppo_cpp_amd import hostapi
    assert hasattr(hostapi.load_host_library(), "ppo_host_learn_masked")
    src = open(os.path.join(HOST, "env", "action_mask.hpp")).read()
    assert "struct IActionMask" in src and "get_action_mask()" in src and "has_action_mask()" in src


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def make(O, A, hidden, seed=0, pi_gain=1.0, masking=False, **overrides):
    import ppo_cpp_amd
    g = ppo_cpp_amd.PPOHip(O, A, list(hidden), action_dist="categorical", **overrides)
    c = g.cfg
    ref = MaskedCatRef(O, A, hidden, ent_coef=c.ent_coef, vf_coef=c.vf_coef, max_grad_norm=c.max_grad_norm, beta1=c.adam_beta1,
                       beta2=c.adam_beta2, eps=c.adam_eps)
    ref.init_random(seed, pi_gain)
    g.set_flat(ref.theta.astype(np.float32))
    if masking:
        g.set_action_masking(True)
        assert g.get_action_masking()
    return ref, g


def near_ties(x):
    """rows whose two best entries (forbidden ones are -inf) are closer than TIE"""
    top2 = np.sort(x, axis=1)[:, -2:]
    with np.errstate(invalid="ignore"):
        return (top2[:, 1] - top2[:, 0]) < TIE


def check_actions(got, want, pert, mask, msg):
    """never forbidden (exact); equal on every row except near-ties of the two best perturbed allowed logits, whose share is printed and bounded"""
    n = len(got)
    gi = got.astype(np.int64)
    assert np.all(got == np.floor(got)) and gi.min() >= 0 and gi.max() < mask.shape[1], msg
    assert np.all(mask[np.arange(n), gi] != 0), "%s: forbidden category chosen on rows %s" % (msg, np.nonzero(mask[np.arange(n), gi] == 0)[0][:5])
    tie = near_ties(pert)
    bad = (got != want) & ~tie
    assert not bad.any(), "%s: %d rows differ (first %s)" % (msg, bad.sum(), np.nonzero(bad)[0][:5])
    print("%s: near-tie rows skipped: %d of %d" % (msg, tie.sum(), n))
    assert tie.sum() <= 0.01 * n, (msg, tie.sum(), n)


@pytest.mark.gpu
@pytest.mark.parametrize("O,A,hidden", [(18, 6, (64, 64)), (18, 18, (256, 256)), (18, 40, (256, 256)), (256, 64, (1024, 1024))])
@pytest.mark.parametrize("n", [1, 17, 300])
def test_masked_step_matches_reference(O, A, hidden, n):
    ref, g = make(O, A, hidden, seed=n)
    rng = np.random.RandomState(7)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    mask = random_masks(rng, n, A)
    a, v, nlp = g.step(obs, u, mask=mask)
    assert a.shape == (n,) and v.shape == (n,) and nlp.shape == (n,)
    ra, rv, rnlp, pert = ref.step(obs, u, mask)
    check_actions(a, ra, pert, mask, "sampled actions")
    logits = ref.forward(obs)[0]
    nlp_all, _, _ = masked_softmax_stats(logits, mask)
    close(nlp, nlp_all[np.arange(n), a.astype(np.int64)], msg="neglogp")
    one = mask.sum(1) == 1
    assert one.any()
    assert np.all(np.abs(nlp[one]) <= 1e-6), nlp[one]
    close(v, rv, msg="value")
    det = g.act_deterministic(obs, mask=mask)
    assert det.shape == (n,)
    check_actions(det, ref.act_deterministic(obs, mask).astype(np.float32), np.where(mask != 0, logits, -np.inf), mask, "deterministic actions")
    # the on-device counter draw under the mask: never forbidden either
    g.seed(3)
    a2, _, nlp2 = g.step(obs, mask=mask)
    assert np.all(mask[np.arange(n), a2.astype(np.int64)] != 0)
    close(nlp2, nlp_all[np.arange(n), a2.astype(np.int64)], msg="neglogp of the counter draw")
    kc = g.kernel_counts()
    assert kc["policy_step_kernel<cat,mask>"] == 3 and kc["policy_step_kernel<cat>"] == 0, kc
    g.close()


def synth_batch(ref, n, seed, mask=None, cr=CR):
    """tests/test_discrete_policy.synth_batch with the actions sampled under `mask`"""
    rng = np.random.RandomState(seed)
    obs = rng.uniform(-1, 1, (n, ref.O)).astype(np.float32)
    a, v, nlp, _ = ref.step(obs, rng.uniform(size=(n, ref.A)), mask)
    old_nlp = (nlp + rng.normal(scale=0.15, size=n)).astype(np.float32)
    old_v = (v + rng.normal(scale=0.2, size=n)).astype(np.float32)
    ret = (v + rng.normal(scale=0.5, size=n)).astype(np.float32)
    ratio = np.exp(old_nlp.astype(np.float64) - nlp)
    near = np.abs(np.abs(ratio - 1.0) - cr) < 1e-3
    old_nlp[near] += np.float32(0.01)
    dvo = v - old_v
    near = np.abs(np.abs(dvo) - cr) < 1e-3
    old_v[near] -= np.float32(0.01) * np.sign(dvo[near]).astype(np.float32)
    dvo = v - old_v
    vclip = old_v + np.clip(dvo, -cr, cr)
    s1, s2 = (v - ret) ** 2, (vclip - ret) ** 2
    near = (np.abs(dvo) > cr) & (np.abs(s1 - s2) < 1e-3 * np.maximum(s1, 1e-6))
    ret[near] += np.float32(0.05)
    adv = ret - old_v
    adv = ((adv - adv.mean()) / (adv.std() + 1e-8)).astype(np.float32)
    return obs, a.astype(np.float32), adv, ret, old_nlp, old_v


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", [(64, 64), (256, 256)])
def test_all_ones_masks_give_the_unmasked_bits(hidden):
    O, A, E, T, nmb, epochs = 18, 18, 32, 8, 4, 2
    ref, g0 = make(O, A, hidden, seed=4, ent_coef=0.01)
    _, g1 = make(O, A, hidden, seed=4, ent_coef=0.01, masking=True)
    rng = np.random.RandomState(5)
    n = 100
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    ones = np.ones((n, A), np.float32)
    for x, y in zip(g0.step(obs, u), g1.step(obs, u, mask=ones)):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(g0.act_deterministic(obs), g1.act_deterministic(obs, mask=ones))
    batch = synth_batch(ref, n, 11)
    np.testing.assert_array_equal(g0.train_step(LR, CR, *batch), g1.train_step(LR, CR, *batch, mask=ones))
    for x, y in zip(g0.last_grad(), g1.last_grad()):
        np.testing.assert_array_equal(x, y)
    for which in range(3):
        np.testing.assert_array_equal(g0.get_flat(which), g1.get_flat(which))
    # a two-epoch update: the same uploaded fields, the masking handle's mask buffer left at its initial ones
    for g in (g0, g1):
        g.norm_init(E)
        g.rollout_alloc(E, T)
    np.testing.assert_array_equal(g1.rollout_get("masks"), np.ones((T, E, A), np.float32))
    obs_r = rng.uniform(-1, 1, (T, E, O)).astype(np.float32)
    a_r, v_r, nlp_r, _ = ref.step(obs_r.reshape(-1, O), rng.uniform(size=(T * E, A)))
    fields = {"obs": obs_r, "actions": a_r.reshape(T, E), "values": v_r.reshape(T, E), "neglogp": nlp_r.reshape(T, E) + rng.normal(scale=0.1, size=(T, E)),
              "returns": v_r.reshape(T, E) + rng.normal(scale=0.5, size=(T, E))}
    perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
    out = []
    for g in (g0, g1):
        for f, x in fields.items():
            g.rollout_set(f, np.asarray(x, np.float32))
        out.append(g.update(LR, CR, epochs, nmb, perms))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    for which in range(3):
        np.testing.assert_array_equal(g0.get_flat(which), g1.get_flat(which))
    kc0, kc1 = g0.kernel_counts(), g1.kernel_counts()
    assert kc0["policy_step_kernel<cat,mask>"] == 0 and kc0["train_fwd_bwd_kernel<cat,mask>"] == 0, kc0
    assert kc1["policy_step_kernel<cat,mask>"] > 0 and kc1["train_fwd_bwd_kernel<cat,mask>"] > 0, kc1
    g0.close(); g1.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,n", [((64, 64), 200), ((256, 256), 512)])
def test_three_masked_train_steps_match_reference(hidden, n):
    O, A, dead = 18, 18, 5
    ref, g = make(O, A, hidden, seed=9, ent_coef=0.01)
    o_w, s_w = ref.offs["pi/w"]
    o_b, _ = ref.offs["pi/b"]
    for it in range(3):
        mask = random_masks(np.random.RandomState(200 + it), n, A, special=False)
        mask[:, dead] = 0.0                                     # one category forbidden in every row
        mask[mask.sum(1) == 0, 0] = 1.0
        batch = synth_batch(ref, n, 100 + it, mask)
        losses = g.train_step(LR, CR, *batch, mask=mask)
        grad, norm = g.last_grad()
        ref_losses, ref_grad = ref.train_step(LR, CR, *batch, mask=mask)
        close(losses[:4], ref_losses[:4], rtol=1e-4, atol=1e-6, msg="losses it=%d" % it)
        assert abs(losses[4] - ref_losses[4]) <= 1.0 / n + 1e-6, ("clipfrac", losses[4], ref_losses[4])
        gs = np.abs(ref_grad).max()
        close(grad, ref_grad, rtol=2e-4, atol=2e-6 * gs, msg="grad it=%d" % it)
        close(norm, np.sqrt(np.dot(ref_grad, ref_grad)), rtol=1e-4, msg="norm it=%d" % it)
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=2e-6, msg="theta it=%d" % it)
        close(g.get_flat(1), ref.m, rtol=2e-4, atol=1e-7 * max(1.0, gs), msg="adam m it=%d" % it)
        gw = grad[o_w:o_w + s_w[0] * s_w[1]].reshape(s_w)
        assert np.all(gw[:, dead] == 0.0) and grad[o_b + dead] == 0.0, "the forbidden category's column / bias entry must get an exactly zero gradient"
        assert np.any(gw[:, dead - 1] != 0.0)
    g.close()


def ref_rollout(ref, seed, E, T, u, masks):
    """runner.hpp:56-157 over the oracle's seeded synthetic env with the masked categorical reference policy (the env ignores the actions)"""
    from oracle import oracle as o
    from oracle import numpy_port as npp
    nz = o.Normalizer(E, ref.O)
    raw, _, _ = o.seeded_env_step(seed, 0, E, 0, ref.O)
    obs, dones = nz.obs(raw), np.zeros(E, np.float32)
    ro = {k: [] for k in ("obs", "actions", "values", "neglogp", "dones", "rewards", "pert", "nlp_all")}
    for t in range(T):
        a, v, nlp, pert = ref.step(obs, u[t], masks[t])
        nlp_all, _, _ = masked_softmax_stats(ref.forward(obs)[0], masks[t])
        for k, x in (("obs", obs), ("actions", a), ("values", v), ("neglogp", nlp), ("dones", dones), ("pert", pert), ("nlp_all", nlp_all)):
            ro[k].append(x)
        raw, rew, dones = o.seeded_env_step(seed, 0, E, t + 1, ref.O)
        obs = nz.obs(raw)
        ro["rewards"].append(nz.reward(rew, dones))
    ro = {k: np.array(x) for k, x in ro.items()}
    _, last_v = ref.forward(obs)
    ro["returns"] = npp.gae(ro["rewards"].astype(np.float32), ro["values"].astype(np.float32), ro["dones"], last_v.astype(np.float32),
                            dones, GAMMA, LAM)
    ro["masks"] = np.asarray(masks, np.float32)
    return ro


@pytest.mark.gpu
@pytest.mark.parametrize("E,T,direct", [(1, 16, True), (1, 16, False), (256, 4, False)])
def test_host_env_loop_with_masks_matches_reference(E, T, direct, monkeypatch):
    """direct: the policy tower's workgroups publish the actions into pinned memory themselves (the library's form for <= 64 environments), counted as
    "policy_step_kernel<host_action>"; the E = 1 case runs both that form and, with PPO_HIP_NO_DIRECT_ACT=1, the copy-engine form; 256 environments take the copy."""
    from oracle import oracle as o
    O, A = 18, 7
    if E == 1 and not direct:
        monkeypatch.setenv("PPO_HIP_NO_DIRECT_ACT", "1")
    else:
        monkeypatch.delenv("PPO_HIP_NO_DIRECT_ACT", raising=False)
    monkeypatch.delenv("PPO_HIP_DIRECT_ACT_MAX_BLOCKS", raising=False)
    ref, g = make(O, A, (64, 64), seed=40 + E, masking=True)
    rng = np.random.RandomState(E + 1)
    u = rng.uniform(size=(T, E, A)).astype(np.float32)
    masks = random_masks(rng, T * E, A, special=False).reshape(T, E, A)
    ro = ref_rollout(ref, 99, E, T, u, masks)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    raw, _, _ = o.seeded_env_step(99, 0, E, 0, O)
    g.rollout_reset(raw)
    acts = []
    for t in range(T):
        a = g.rollout_act(t, u[t], mask=masks[t])
        assert a.shape == (E,)
        acts.append(a)
        raw, rew, dn = o.seeded_env_step(99, 0, E, t + 1, O)
        g.rollout_observe(t, raw, rew, dn)
    g.rollout_finish(GAMMA, LAM)
    got = {f: g.rollout_get(f) for f in ("obs", "actions", "values", "neglogp", "rewards", "returns", "masks")}
    np.testing.assert_array_equal(got["masks"], masks)
    np.testing.assert_array_equal(np.array(acts), got["actions"])
    check_actions(got["actions"].reshape(-1), ro["actions"].reshape(-1).astype(np.float32), ro["pert"].reshape(T * E, -1), masks.reshape(T * E, A),
                  "host Env E=%d actions" % E)
    for f in ("obs", "values", "rewards", "returns"):
        close(got[f], ro[f], rtol=2e-4, atol=2e-5, msg=f)
    want = np.take_along_axis(ro["nlp_all"].reshape(T * E, -1), got["actions"].reshape(-1, 1).astype(np.int64), 1).reshape(T, E)
    close(got["neglogp"], want, rtol=2e-4, atol=2e-5, msg="neglogp")
    kc = g.kernel_counts()
    assert kc["policy_step_kernel<cat,mask>"] == T
    assert kc["policy_step_kernel<host_action>"] == (T if direct else 0), kc
    # the plain call on a masking handle records an all-ones row
    g.rollout_act(0, u[0])
    np.testing.assert_array_equal(g.rollout_get("masks")[0], np.ones((E, A), np.float32))
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,E,T,nmb", [((64, 64), 32, 16, 4), ((256, 256), 256, 8, 4)])
def test_two_masked_updates_with_explicit_perms_match_reference(hidden, E, T, nmb):
    O, A, epochs = 18, 18, 2
    ref, g = make(O, A, hidden, seed=17, ent_coef=0.01, masking=True)
    _, plain = make(O, A, hidden, seed=17, ent_coef=0.01)
    for h in (g, plain):
        h.norm_init(E)
        h.rollout_alloc(E, T)
    rng = np.random.RandomState(3)
    for it in range(2):
        u = rng.uniform(size=(T, E, A)).astype(np.float32)
        masks = random_masks(rng, T * E, A, special=False).reshape(T, E, A)
        ro = ref_rollout(ref, 500 + it, E, T, u, masks)
        ro["neglogp"] = (ro["neglogp"] + rng.normal(scale=0.1, size=(T, E))).astype(np.float32)   # move the ratio off 1
        fields = ("obs", "actions", "values", "neglogp", "returns", "masks")
        for f in fields:
            g.rollout_set(f, np.asarray(ro[f], np.float32))
        perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
        rows, mean = g.update(LR, CR, epochs, nmb, perms)
        ref_rows, ref_mean = ref.update({f: np.asarray(ro[f], np.float32) for f in fields}, perms, nmb, LR, CR)
        close(rows[:, :4], ref_rows[:, :4], rtol=1e-4, atol=1e-6, msg="loss rows update %d" % it)
        assert np.all(np.abs(rows[:, 4] - ref_rows[:, 4]) <= nmb / (E * T) + 1e-6)
        close(mean[:4], ref_mean[:4], rtol=1e-4, atol=1e-6, msg="mean losses update %d" % it)
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=5e-6, msg="theta after update %d" % it)
        nodes = g.debug_graph_nodes()
        assert nodes is not None and nodes["kernel"] > 0, nodes
        assert nodes["memset"] == 0 and nodes["memcpy"] == 0 and nodes["other"] == 0, nodes
    kc = g.kernel_counts()
    assert kc["train_fwd_bwd_kernel<cat,mask>"] > 0 and kc["train_fwd_bwd_kernel<cat>"] == 0, kc
    g.step(np.zeros((3, O), np.float32), mask=np.ones((3, A), np.float32))
    assert g.kernel_counts()["policy_step_kernel<cat,mask>"] > 0
    # a categorical handle without masking in the same test: the masked variants never run
    for f in ("obs", "actions", "values", "neglogp", "returns"):
        plain.rollout_set(f, np.asarray(ro[f], np.float32))
    plain.update(LR, CR, epochs, nmb, perms)
    plain.step(np.zeros((3, O), np.float32))
    kp = plain.kernel_counts()
    assert kp["policy_step_kernel<cat,mask>"] == 0 and kp["train_fwd_bwd_kernel<cat,mask>"] == 0, kp
    assert kp["policy_step_kernel<cat>"] > 0 and kp["train_fwd_bwd_kernel<cat>"] > 0, kp
    g.close(); plain.close()


@pytest.mark.gpu
def test_mask_errors():
    import ppo_cpp_amd
    Err = ppo_cpp_amd.PPOHipError
    O, A, n = 18, 6, 32
    obs0 = np.zeros((4, O), np.float32)
    gauss = ppo_cpp_amd.PPOHip(O, A, [64, 64])
    with pytest.raises(Err, match="categorical"):
        gauss.set_action_masking(True)
    with pytest.raises(Err, match="categorical"):
        gauss.step(obs0, mask=np.ones((4, A), np.float32))
    gauss.close()
    bf = ppo_cpp_amd.PPOHip(O, A, [256, 256], compute_dtype=1)
    with pytest.raises(Err, match="categorical"):
        bf.set_action_masking(True)
    with pytest.raises(Err, match="categorical"):
        bf.act_deterministic(obs0, mask=np.ones((4, A), np.float32))
    bf.close()

    ref, g = make(O, A, (64, 64))
    ones = np.ones((n, A), np.float32)
    obs, a, adv, ret, nlp, v = synth_batch(ref, n, 0, ones)
    zero_row = ones.copy(); zero_row[7] = 0.0
    theta = g.get_flat(0)
    with pytest.raises(Err, match="allows no category"):
        g.step(obs, mask=zero_row)
    with pytest.raises(Err, match="allows no category"):
        g.act_deterministic(obs, mask=zero_row)
    with pytest.raises(Err, match="allows no category"):
        g.train_step(LR, CR, obs, a, adv, ret, nlp, v, mask=zero_row)
    forbid = ones.copy(); forbid[5, int(a[5])] = 0.0
    with pytest.raises(Err, match="forbidden by the row's own mask"):
        g.train_step(LR, CR, obs, a, adv, ret, nlp, v, mask=forbid)
    np.testing.assert_array_equal(g.get_flat(0), theta)          # nothing was trained
    # masking off: no field 8, no masked rollout step
    E, T = 4, 2
    g.norm_init(E)
    g.rollout_alloc(E, T)
    g.rollout_reset(np.zeros((E, O), np.float32))
    with pytest.raises(Err, match="masking"):
        g.rollout_get("masks")
    with pytest.raises(Err, match="masking"):
        g.rollout_set("masks", np.ones((T, E, A), np.float32))
    with pytest.raises(Err, match="masking is off"):
        g.rollout_act(0, mask=np.ones((E, A), np.float32))
    g.rollout_act(0)
    # the setting changed: the rollout is gone until the next rollout_alloc
    g.set_action_masking(True)
    for call in (lambda: g.rollout_act(0), lambda: g.rollout_get("masks"), lambda: g.rollout_reset(np.zeros((E, O), np.float32)),
                 lambda: g.rollout_finish(GAMMA, LAM), lambda: g.update(LR, CR, 1, 1)):
        with pytest.raises(Err, match="no rollout allocated"):
            call()
    g.rollout_alloc(E, T)
    g.rollout_reset(np.zeros((E, O), np.float32))
    bad = np.ones((E, A), np.float32); bad[2] = 0.0
    with pytest.raises(Err, match="allows no category"):
        g.rollout_act(0, mask=bad)
    up = np.ones((T, E, A), np.float32); up[1, 3] = 0.0
    with pytest.raises(Err, match="allows no category"):
        g.rollout_set("masks", up)
    np.testing.assert_array_equal(g.rollout_get("masks"), np.ones((T, E, A), np.float32))
    g.rollout_act(0, mask=np.ones((E, A), np.float32))
    g.set_action_masking(False)
    with pytest.raises(Err, match="no rollout allocated"):
        g.rollout_act(0)
    g.train_step(LR, CR, obs, a, adv, ret, nlp, v, mask=ones)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("reference_loop", [False, True])
def test_ppo2_learns_the_masked_target_task(reference_loop):
    """Learning through PPO2::learn: MaskedTargetEnv x 16 (host/env/env_mock.hpp: DiscreteTargetEnv's task, about half of the 18 categories forbidden at every
    step, reward 1 / 0 / -1 for the target / another allowed / a forbidden category) behind VecEnv + EnvNormalize, 64 steps, [64,64], 150 updates of
    4 epochs x 4 minibatches at lr 2e-3 -- the settings of test_ppo2_learns_the_discrete_target_task.  PPO2 finds the IActionMask mixin by itself; the
    HBM-resident loop samples through ppo_rollout_act_masked, the literal loop (reference_loop) through ppo_step_masked / ppo_train_step_masked.
    The environments must have received NO forbidden action over the whole run (exact), and the deterministic playback must be legal too.
    A uniform policy over the allowed categories earns about 1/9.5 = 0.105.  The NumPy reference loop (tests/masked_categorical_ref.masked_learn_loop with the
    oracle's EnvNormalize, fed the environments' own stream -- the host program's `dump` above) over three draw seeds: first-15 -> last-15 mean reward
    0.191 -> 0.586, 0.189 -> 0.602, 0.188 -> 0.580, no forbidden action.
    RISE = 0.26: the last-15 mean over the first-15; two thirds of the reference's smallest rise (0.392).
    BAND = 0.09: |last-15 mean - 0.589| (the reference's mean over the seeds); four times the 0.022 its seeds spread by, because the two legs differ in
    initial weights and draws.
    GPU_FIGURES
    """
    from ppo_cpp_amd import hostapi
    RISE, BAND, REF_LAST15 = 0.26, 0.09, 0.589
    got = hostapi.learn_masked(16, 64, [64, 64], 150, 4, 4, 2e-3, 0.2, seed=11, act_dim=18, reference_loop=reference_loop, n_playback=50)
    assert got["forbidden_received"] == 0, got["forbidden_received"]
    assert np.all(got["playback_legal"] == 1.0), got["playback_actions"]
    c = got["reward_curve"]
    first, last = c[:15].mean(), c[-15:].mean()
    print("reference_loop=%s reward curve first-15 %.3f last-15 %.3f" % (reference_loop, first, last))
    assert last - first >= RISE, (first, last)
    assert abs(last - REF_LAST15) <= BAND, (last, REF_LAST15)
