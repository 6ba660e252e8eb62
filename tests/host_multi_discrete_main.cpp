// A stand-alone host program (no GPU, no Python): MultiDiscreteTargetEnv x 3 through TimeLimit + VecEnv + EnvNormalize (host/env/multi_discrete.hpp).
// EnvNormalize's arithmetic lives in libppo_hip; this program brings pass-through stand-ins for the few ppo_norm_* calls instead of linking the library, so that it
// runs where no device is.  tests/test_multi_discrete.py compiles and runs it; it prints "ok" and returns 0, or says what failed.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "env/env_mock.hpp"
#include "env/env_normalize.hpp"
#include "env/time_limit.hpp"
#include "env/vec_env.hpp"

extern "C" {
static int g_norm_envs = 0;
int ppo_norm_init(ppo_handle*, int32_t n_envs, float, float, float, float) { g_norm_envs = n_envs; return 0; }
int ppo_norm_set_flags(ppo_handle*, int, int) { return 0; }
int ppo_norm_obs(ppo_handle*, const float* raw, int32_t, int, float* out) { (void)raw; (void)out; return 0; }      // (EnvNormalize hands over a copy: pass-through)
int ppo_norm_reward(ppo_handle*, const float*, const float*, int32_t, int, float*) { return 0; }
int ppo_norm_reset_returns(ppo_handle*) { return 0; }
int ppo_norm_get_stats(ppo_handle*, int, float*, float*, double*) { return 0; }
int ppo_norm_set_stats(ppo_handle*, int, const float*, const float*, double) { return 0; }
const char* ppo_last_error(const ppo_handle*) { return "stand-in"; }
}

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

template <class F>
static bool throws(F&& f) { try { f(); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); return true; } return false; }

int main() {
    const std::vector<int> nvec = {3, 5, 2};
    const int n = 3, O = 7, K = 3, A = 10, limit = 4;
    // ---- TimeLimit inside VecEnv inside EnvNormalize: the components are forwarded at every level ----
    std::vector<std::shared_ptr<MultiDiscreteTargetEnv>> kids;
    std::vector<std::shared_ptr<Env>> envs;
    for (int i = 0; i < n; ++i) {
        kids.push_back(std::make_shared<MultiDiscreteTargetEnv>(77u, (uint32_t)i, O, nvec, 100));
        envs.push_back(std::make_shared<TimeLimit>(kids.back(), limit));
        CHECK(action_nvec_of(envs.back().get()) == nvec);
    }
    {
        EnvNormalize env{std::unique_ptr<Env>(new VecEnv(envs, 2)), nullptr, /*training=*/true};
        CHECK(g_norm_envs == n);
        CHECK(env.get_action_space() == Env::SPACE_DISCRETE);
        CHECK(env.get_action_space_size() == A && env.get_num_envs() == n && env.get_observation_space_size() == O);
        CHECK(env.has_action_nvec() && env.get_action_nvec() == nvec);
        CHECK(action_nvec_of(&env) == nvec && action_nvec_of(&env.inner()) == nvec);
        CHECK(!env.has_action_mask());
        const Mat ones = env.get_action_mask();                         // nothing inside masks: all allowed, [n, A]
        CHECK(ones.rows() == n && ones.cols() == A);
        for (long i = 0; i < (long)n * A; ++i) CHECK(ones.data()[i] == 1.f);
        Mat obs = env.reset();
        CHECK(obs.rows() == n && obs.cols() == O);
        for (int t = 0; t < 2 * limit; ++t) {
            Mat act(n, K);                                              // every environment's targets: reward 1 (all K components hit)
            for (int i = 0; i < n; ++i) { const std::vector<int> tg = kids[i]->targets(); for (int k = 0; k < K; ++k) act(i, k) = (float)tg[k]; }
            if (t == 1) act(1, 2) = (float)(1 - (int)act(1, 2));        // one component of environment 1 misses once: 2 of 3
            const std::vector<Mat> r = env.step(act);
            CHECK(r[0].rows() == n && r[0].cols() == O && r[1].rows() == n && r[2].rows() == n);
            const Mat raw = env.get_original_rew();
            for (int i = 0; i < n; ++i) {
                const float want = (t == 1 && i == 1) ? 2.f / 3.f : 1.f;
                CHECK(raw(i, 0) == want);
                CHECK(r[2](i, 0) == ((t + 1) % limit == 0 ? 1.f : 0.f));
                CHECK(env.get_truncated()(i, 0) == r[2](i, 0));            // every done here is the time limit's
            }
        }
    }
    // ---- the masked variant: [n, A] masks, every component keeps its target ----
    {
        std::vector<std::shared_ptr<MultiDiscreteTargetEnv>> mk;
        std::vector<std::shared_ptr<Env>> menvs;
        for (int i = 0; i < n; ++i) { mk.push_back(std::make_shared<MultiDiscreteTargetEnv>(77u, (uint32_t)i, O, nvec, 100, true)); menvs.push_back(mk.back()); }
        EnvNormalize env{std::unique_ptr<Env>(new VecEnv(menvs, 2)), nullptr, /*training=*/true};
        CHECK(env.has_action_mask() && env.get_action_nvec() == nvec);
        env.reset();
        long forbidden_cells = 0;
        for (int t = 0; t < 20; ++t) {
            const Mat m = env.get_action_mask();
            CHECK(m.rows() == n && m.cols() == A);
            Mat act(n, K);
            for (int i = 0; i < n; ++i) {
                const std::vector<int> tg = mk[i]->targets();
                for (int k = 0, o = 0; k < K; o += nvec[k], ++k) {
                    CHECK(m(i, o + tg[k]) == 1.f);                      // the target is never forbidden
                    for (int j = 0; j < nvec[k]; ++j) forbidden_cells += m(i, o + j) == 0.f;
                    act(i, k) = (float)tg[k];
                }
            }
            if (t == 3) {                                               // send environment 0 a forbidden category if its mask has one: reward -1, counted
                const Mat m0 = m;
                for (int j = 0; j < nvec[1]; ++j) if (m0(0, nvec[0] + j) == 0.f) { act(0, 1) = (float)j; break; }
            }
            env.step(act);
        }
        CHECK(forbidden_cells > 0);
        long sent = 0;
        for (const auto& k : mk) sent += k->forbidden_received();
        CHECK(sent <= 1);
        if (sent == 1) CHECK(mk[0]->forbidden_received() == 1);
    }
    // ---- children that disagree are refused; children without the mixin are not multi-discrete ----
    {
        std::vector<std::shared_ptr<Env>> bad = {std::make_shared<MultiDiscreteTargetEnv>(1u, 0u, O, nvec), std::make_shared<MultiDiscreteTargetEnv>(1u, 1u, O, std::vector<int>{5, 3, 2})};
        CHECK(throws([&] { VecEnv v(bad, 1); }));
        std::vector<std::shared_ptr<Env>> mixed = {std::make_shared<MultiDiscreteTargetEnv>(1u, 0u, O, nvec), std::make_shared<DiscreteTargetEnv>(1u, 1u, O, A)};
        CHECK(throws([&] { VecEnv v(mixed, 1); }));
        std::vector<std::shared_ptr<Env>> plain = {std::make_shared<DiscreteTargetEnv>(1u, 0u, O, A), std::make_shared<DiscreteTargetEnv>(1u, 1u, O, A)};
        VecEnv v(plain, 1);
        CHECK(!v.has_action_nvec() && action_nvec_of(&v).empty());
    }
    std::printf("ok\n");
    return 0;
}
