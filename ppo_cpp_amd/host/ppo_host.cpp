// ppo_host.cpp -- C entry points over the C++ host layer (env stack, Runner, PPO2) so that tests and bench.py can
// drive it with ctypes.  The wiring of ppo_host_learn mirrors the reference's main() (ppo2.cpp:188-250):
//   N x Env -> VecEnv -> EnvNormalize{training} -> PPO2{gamma .99, lam .95, vf .5, max_grad_norm .5, 32 minibatches}.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <regex>
#include <thread>

#include "env/env_mock.hpp"
#include "env/env_normalize.hpp"
#include "env/time_limit.hpp"
#include "env/vec_env.hpp"
#include "ppo2/checkpoint.hpp"
#include "ppo2/graph_spec.hpp"
#include "ppo2/ppo2.hpp"

extern "C" {

// Port of the reference's only test (test/vecenv_test.cpp:13-49): N x EnvMock(i+1) behind a VecEnv, `steps` steps of
// zero actions; every observation column and the reward column must equal [1..N]^T.  Returns 0 or the failing check.
int ppo_host_vecenv_check(int num_envs, int steps, int max_workers) {
    std::vector<std::shared_ptr<Env>> envs;
    Mat expect = Mat::Zero(num_envs, 1);
    for (int i = 0; i < num_envs; ++i) { envs.push_back(std::make_shared<EnvMock>(i + 1)); expect(i, 0) = (float)(i + 1); }
    VecEnv ve{envs, max_workers};
    for (int s = 0; s < steps; ++s) {
        const Mat actions = Mat::Zero(ve.get_num_envs(), ve.get_action_space_size());
        const std::vector<Mat> result = ve.step(actions);
        const Mat& obs = result[0];
        const Mat& rew = result[1];
        if (obs.rows() != ve.get_num_envs()) return 1;
        if (rew.rows() != ve.get_num_envs()) return 2;
        if (obs.cols() != ve.get_observation_space_size()) return 3;
        if (rew.cols() != 1) return 4;
        if ((rew - expect).squaredNorm() > 1e-2f) return 5;
        for (int j = 0; j < ve.get_observation_space_size(); ++j)
            if ((obs.col(j) - expect).squaredNorm() > 1e-2f) return 6;
        const Mat dones = result[2];
        for (int i = 0; i < num_envs; ++i) if (dones(i, 0) != ((s + 1) % 300 == 0 ? 1.f : 0.f)) return 7;
        if ((ve.get_original_rew() - expect).squaredNorm() > 1e-2f) return 8;
    }
    const Mat r = ve.reset();                         // gathers get_original_obs(), does not reset sub-envs
    if (r.rows() != num_envs || r.cols() != 18) return 9;
    for (int i = 0; i < num_envs; ++i) if (r(i, 0) != (float)(i + 1)) return 10;
    return 0;
}

// pure host checks of the small utilities (no GPU): Mat shim, JSON, episode logger, env-major flatten
int ppo_host_selftest() {
    {   // flatten: [T,E,W] -> row e*T+t
        const int T = 3, E = 2, W = 2;
        float src[T * E * W];
        for (int i = 0; i < T * E * W; ++i) src[i] = (float)i;
        auto m = Runner::flatten(src, T, E, W);
        for (int e = 0; e < E; ++e) for (int t = 0; t < T; ++t) for (int w = 0; w < W; ++w)
            if ((*m)(e * T + t, w) != src[(t * E + e) * W + w]) return 1;
    }
    {   // episode logger: env 0 has a done at k=2 -> episode reward = acc + r0 + r1, new accumulator r2 + r3
        Mat acc = Mat::Zero(2, 1), rew(2, 4), dn = Mat::Zero(2, 4);
        acc(0, 0) = 10.f;
        for (int e = 0; e < 2; ++e) for (int k = 0; k < 4; ++k) rew(e, k) = (float)(k + 1);
        dn(0, 2) = 1.f;
        std::vector<std::pair<int, float>> got;
        acc = Utils::total_episode_reward_logger(acc, rew, dn, [&](int s, const char*, float v) { got.push_back({s, v}); }, 100);
        if (got.size() != 1 || got[0].first != 102 || got[0].second != 13.f) return 2;
        if (acc(0, 0) != 7.f || acc(1, 0) != 10.f) return 3;
    }
    {   // JSON round trip in the reference's running-statistics format
        nlohmann::json j;
        j["obs_rms"]["mean"] = std::vector<float>{0.5f, -1.25f};
        j["obs_rms"]["count"] = 72001473.000001;
        const std::string text = j.dump();
#ifndef PPO_HAVE_NLOHMANN
        nlohmann::json k = nlohmann::json::parse(text);
        if (k["obs_rms"]["mean"].get<std::vector<float>>()[1] != -1.25f) return 4;
        if (std::fabs(k["obs_rms"]["count"].get<double>() - 72001473.000001) > 1e-6) return 5;
#endif
    }
    {   // seeded mock: deterministic, bounded
        SeededEnvMock a(1234, 7), b(1234, 7);
        const Mat o1 = a.reset(), o2 = b.reset();
        for (int j = 0; j < 18; ++j) if (o1(0, j) != o2(0, j) || o1(0, j) < -1.f || o1(0, j) >= 1.f) return 6;
    }
    return 0;
}

// read a reference checkpoint (<in_prefix>.index / .data-00000-of-00001) and write it back under out_prefix; returns the
// number of tensors, or -1 (message on stderr).  tests/test_checkpoint.py compares the output files byte for byte.
int ppo_host_bundle_roundtrip(const char* in_prefix, const char* out_prefix) {
    try {
        const ckpt::Bundle b = ckpt::load_bundle(in_prefix);
        ckpt::save_bundle(out_prefix, b);
        return (int)b.size();
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return -1; }
}

// tensor access for tests: copies tensor `name` (at most cap floats) and its shape (up to 4 dims); returns element count
int ppo_host_bundle_tensor(const char* prefix, const char* name, float* dst, int cap, long long shape[4]) {
    try {
        const ckpt::Bundle b = ckpt::load_bundle(prefix);
        auto it = b.find(name);
        if (it == b.end()) return -2;
        const int n = (int)it->second.data.size();
        if (n > cap) return -3;
        std::memcpy(dst, it->second.data.data(), sizeof(float) * (size_t)n);
        for (int i = 0; i < 4; ++i) shape[i] = i < (int)it->second.shape.size() ? it->second.shape[i] : 0;
        return n;
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return -1; }
}

// PPO2::load of a reference checkpoint ([4,5] net, EnvMock behind EnvNormalize) -> deterministic action + value of the
// zero observation -> PPO2::save under out_prefix.  Returns 0; mu[18], value[1], obs_count out.
int ppo_host_checkpoint_eval(const char* in_prefix, const char* out_prefix, float* mu, double* obs_count) {
    ppo_handle* h = nullptr;
    try {
        ppo_config cfg; const int32_t hidden[2] = {4, 5};
        ppo_config_default(&cfg, 18, 18, 2, hidden);
        if (ppo_create(&cfg, &h) != 0) throw std::runtime_error(ppo_last_error(nullptr));
        {
            EnvNormalize env{std::unique_ptr<Env>(new EnvMock(1)), h, /*training=*/false};
            PPO2 algo{h, env};
            algo.load(in_prefix);
            const Mat a = algo.eval(Mat::Zero(1, 18));
            std::memcpy(mu, a.data(), sizeof(float) * 18);
            float m[18], v[18];
            if (ppo_norm_get_stats(h, 0, m, v, obs_count) != 0) throw std::runtime_error(ppo_last_error(h));
            algo.save(out_prefix);
        }
        ppo_destroy(h);
        return 0;
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); if (h) ppo_destroy(h); return -1; }
}

// Graph-spec importer: parses a reference .meta.txt; fills cfg, the betas' initial powers, and copies
// variable `name`'s initial value (cap floats).  Returns the element count, -2 if absent, -1 on parse errors.
int ppo_host_graph_spec(const char* path, ppo_config* cfg, float pw0[2], const char* name, float* dst, int cap) {
    try {
        const graphspec::GraphSpec g = graphspec::load_graph_spec(path);
        *cfg = g.config; pw0[0] = g.beta1_power0; pw0[1] = g.beta2_power0;
        if (!name || !name[0]) return 0;
        auto it = g.initial.find(name);
        if (it == g.initial.end()) return -2;
        const int n = (int)it->second.data.size();
        if (n > cap) return -3;
        std::memcpy(dst, it->second.data.data(), sizeof(float) * (size_t)n);
        return n;
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return -1; }
}

// load_graph + Run("init") on the DEVICE (session_creator.hpp:40-58): create a handle from a graph file, assign the graph's
// initial weights, and evaluate deterministic action [n,A], value [n] and the beta powers for the given observations.
int ppo_host_graph_eval(const char* path, const float* obs, int n, float* actions, float* values, float pw[2]) {
    ppo_handle* h = nullptr;
    try {
        const graphspec::GraphSpec g = graphspec::load_graph_spec(path);
        h = graphspec::create_from_graph(g);
        if (ppo_act_deterministic(h, obs, n, actions) != 0 || ppo_value(h, obs, n, values) != 0 || ppo_get_beta_powers(h, pw) != 0)
            throw std::runtime_error(ppo_last_error(h));
        ppo_destroy(h);
        return 0;
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); if (h) ppo_destroy(h); return -1; }
}

struct ppo_host_args {
    int n_envs, n_steps, n_hidden, hidden[8];
    int nminibatches, noptepochs, n_updates;
    float lr, cliprange, gamma, lam;
    int seeded_env;          // 0: EnvMock(i+1) (degenerate constant data, the reference's stub) ; 1: SeededEnvMock ; 2: TargetEnv (learnable: tests/test_learning.py) ;
                             // 3: DiscreteTargetEnv (act_dim categories, a categorical handle: tests/test_discrete_policy.py)
    int device;
    int max_workers;
    int reference_loop;      // 1: force the literal reference loop (Runner::run + host shuffle + _train_step)
    int norm_obs, norm_reward;   // EnvNormalize constructor flags (env_normalize.hpp:24-27)
    unsigned long long seed;     // PPO2::seed (exploration noise + epoch shuffles)
    int obs_dim, act_dim;        // SeededEnvMock's shape (0 = 18): 36 / 18 is the hexapod with observed velocities (hexapod_closed_loop_env.hpp:20)
    float cliprange_vf;          // PPO2's cliprange_vf: < 0 = clip the value with cliprange (the default, -1), >= 0 = its own range, +inf = no value clipping
    int discrete_kernels;        // a discrete Env's handle: 0 = the generic categorical kernels (the default), 1 = PPO_ACT_SHAPE_KERNELS (PPO2::action_dist_for; a multi-discrete Env's: PPO2::create_handle), 2 = PPO_ACT_PAIR_KERNELS (a multi-discrete Env's: PPO2::create_handle's extra_flags), 3 = "binary narrow": PPO_ACT_BINARY_SHAPE_KERNELS as extra_flags of a multi-binary Env's handle (ppo_host_learn_binary, ppo_host_binary_checkpoint_ex; every other entry treats 3 as 0), 4 = "binary pair": PPO_ACT_BINARY_PAIR_KERNELS as extra_flags of the same two entries' handles (every other entry treats 4 as 0)
    int compute_dtype;           // ppo_config::compute_dtype (0 = PPO_F32, the default; 1 = PPO_BF16: a discrete Env's handle is then created with PPO_ACT_BF16_HEAD, a multi-discrete Env's with PPO_ACT_BF16_MULTI_HEAD)
    int n_components, nvec[16];  // ppo_host_learn_multi: the components of MultiDiscreteTargetEnv (act_dim is their sum)
    int multi_masked;            // ppo_host_learn_multi: the environments also carry IActionMask
    int host_step_fused;         // ppo_set_host_step_fused(h, 1) on the created handle before PPO2 sees it: the one-launch host-Env step of a narrow discrete handle (discrete_kernels == 1, <= 32 environments); nothing changes anywhere else
};
// ppo_set_rollout_resident(h, 1) on the handle the next learn entry creates (run_learn, the masked and the multi entry), directly behind the host_step_fused line:
// the resident rollout of a narrow discrete handle (discrete_kernels == 1, <= 64 environments); nothing changes anywhere else.  A process-wide default set through
// ppo_host_set_rollout_resident, not a member of ppo_host_args: that struct's layout and last member are pinned by tests/test_narrow_host_step.py.
static int g_rollout_resident = 0;
void ppo_host_set_rollout_resident(int on) { g_rollout_resident = on != 0; }
// ppo_kernel_counts of the handle of the last ppo_host_learn_masked run, taken before the handle is destroyed (that entry has no count outputs of its own)
static char g_last_count_names[64][32];
static long long g_last_counts[64];
static int g_last_n_counts = 0;
static void keep_kernel_counts(ppo_handle* h) {
    int64_t c64[64];
    g_last_n_counts = ppo_kernel_counts(h, 64, g_last_count_names, c64);
    if (g_last_n_counts < 0) g_last_n_counts = 0;
    for (int i = 0; i < g_last_n_counts; ++i) g_last_counts[i] = (long long)c64[i];
}
int ppo_host_last_kernel_counts(int max, char (*names)[32], long long* counts) {
    const int n = g_last_n_counts < max ? g_last_n_counts : max;
    for (int i = 0; i < n; ++i) { std::memcpy(names[i], g_last_count_names[i], 32); counts[i] = g_last_counts[i]; }
    return n;
}
// the handle's action_dist for `env`: PPO2's choice, plus the opt-ins: the [256,256] pair for a categorical head, the one such a head needs on the bf16 path
static int32_t host_action_dist(Env& env, const ppo_host_args* a) {
    int32_t d = PPO2::action_dist_for(env, a->discrete_kernels == 1);
    if (a->discrete_kernels == 2 && (d & 0xff) == PPO_ACT_CATEGORICAL) d |= PPO_ACT_PAIR_KERNELS;
    return (a->compute_dtype == PPO_BF16 && (d & 0xff) == PPO_ACT_CATEGORICAL) ? (d | PPO_ACT_BF16_HEAD) : d;
}
struct ppo_host_result {
    double env_steps_per_s, collect_ms, update_ms;
    float losses[5];
    int fps_last;
    char error[256];
    double obs_count, ret_count;     // running-statistics counts after the run (1e-6 = never updated)
    double phase_env_ms, phase_act_ms, phase_observe_ms;   // host-Env collect split per update: Env::step | ppo_rollout_act (kernel + D2H + sync) | ppo_rollout_observe (pack + H2D enqueue)
    int pool_workers, pool_chunk, pool_active;              // what the pooled VecEnv settled on: threads incl. the caller, environments per claimed chunk, threads that took part in the last step
};

// explicit inputs / extra outputs of a parity run (all optional)
struct ppo_host_explicit {
    const float* theta_in;       // [P] dense initial weights (null: ppo_init_orthogonal(0))
    const float* noise;          // [n_updates][n_steps][n_envs][A]
    const int32_t* perms;        // [n_updates][noptepochs][n_batch]
    float* losses_out;           // [n_updates][5] mean losses of every update (ppo2.hpp:335)
    float* theta_out;            // [P]
    float* obs_mean; float* obs_var; double* obs_count;      // obs_rms [18], [18], [1]
    float* ret_mean; float* ret_var; double* ret_count;      // ret_rms [1], [1], [1]
    float* reward_curve;         // [n_updates] mean un-normalised reward of every update's rollout
    char (*count_names)[32]; long long* counts; int* n_counts;     // ppo_kernel_counts of the run's handle after learn(): up to 64 entries (all three or none)
    int* applied_out;            // [n_updates][2] Adam steps applied / train steps of every update (target-KL early stopping)
    float target_kl;             // PPO2::set_target_kl: target-KL early stopping, 0 = off.  (Here and not in ppo_host_args: that struct's last member is pinned by
                                 // tests/test_narrow_host_step.py)
};

static int run_learn(const ppo_host_args* a, ppo_host_result* out, const ppo_host_explicit* x) {
    std::memset(out, 0, sizeof *out);
    ppo_handle* h = nullptr;
    try {
        ppo_config cfg;
        const int O = a->obs_dim > 0 ? a->obs_dim : 18, A = a->act_dim > 0 ? a->act_dim : 18;
        if ((O != 18 || A != 18) && !a->seeded_env) throw std::runtime_error("EnvMock (the reference's stub) is 18 / 18");
        ppo_config_default(&cfg, O, A, a->n_hidden, a->hidden);
        cfg.device = a->device;
        auto make_probe = [&]() -> Env* {        // (what the handle's head is chosen from: one environment of the kind the run uses)
            if (a->seeded_env == 3) return new DiscreteTargetEnv(1234u, 0, O, A);
            if (a->seeded_env == 2) return new TargetEnv(1234u, 0, O, A);
            if (a->seeded_env) return new SeededEnvMock(1234u, 0, O, A);
            return new EnvMock(1);
        };
        { std::unique_ptr<Env> probe(make_probe());
          cfg.compute_dtype = a->compute_dtype;
          if (ppo_create_ex(&cfg, host_action_dist(*probe, a), &h) != 0) throw std::runtime_error(ppo_last_error(nullptr)); }
        if (ppo_init_orthogonal(h, 0) != 0) throw std::runtime_error(ppo_last_error(h));
        if (a->host_step_fused && ppo_set_host_step_fused(h, 1) != 0) throw std::runtime_error(ppo_last_error(h));
        if (g_rollout_resident && ppo_set_rollout_resident(h, 1) != 0) throw std::runtime_error(ppo_last_error(h));
        if (x && x->theta_in && ppo_set_flat(h, 0, x->theta_in, ppo_num_params(h)) != 0) throw std::runtime_error(ppo_last_error(h));
        std::vector<std::shared_ptr<Env>> envs;
        auto make_env = [&](uint32_t i) -> Env* {
            if (a->seeded_env == 3) return new DiscreteTargetEnv(1234u, i, O, A);
            if (a->seeded_env == 2) return new TargetEnv(1234u, i, O, A);
            if (a->seeded_env) return new SeededEnvMock(1234u, i, O, A);
            return new EnvMock(i + 1);
        };
        for (int i = 0; i < a->n_envs; ++i) envs.push_back(std::shared_ptr<Env>(make_env((uint32_t)i)));
        std::unique_ptr<Env> inner;
        VecEnv* pool = nullptr;
        if (a->n_envs > 1) inner.reset(pool = new VecEnv(envs, a->max_workers));
        else inner.reset(make_env(0));
        {
            EnvNormalize env{std::move(inner), h, /*training=*/true, a->norm_obs != 0, a->norm_reward != 0, 10.f, 10.f, a->gamma};
            PPO2 algorithm{h, env, a->gamma, a->n_steps, cfg.ent_coef, a->lr, 0.5f, 0.5f, a->lam, a->nminibatches, a->noptepochs, a->cliprange, a->cliprange_vf};
            algorithm.quiet = true;
            struct Plain : Env {       // hides the EnvNormalize type to force the reference loop
                Env& e; explicit Plain(Env& x) : e(x) {}
                std::string get_action_space() override { return e.get_action_space(); }
                std::string get_observation_space() override { return e.get_observation_space(); }
                int get_action_space_size() override { return e.get_action_space_size(); }
                int get_observation_space_size() override { return e.get_observation_space_size(); }
                int get_num_envs() override { return e.get_num_envs(); }
                Mat reset() override { return e.reset(); }
                std::vector<Mat> step(const Mat& x) override { return e.step(x); }
                void render() override {}
                float get_time() override { return 0; }
                Mat get_original_obs() override { return e.get_original_obs(); }
                Mat get_original_rew() override { return e.get_original_rew(); }
                void serialize(nlohmann::json& j) override { e.serialize(j); }
                void deserialize(nlohmann::json& j) override { e.deserialize(j); }
            } plain{env};
            PPO2 literal{h, plain, a->gamma, a->n_steps, cfg.ent_coef, a->lr, 0.5f, 0.5f, a->lam, a->nminibatches, a->noptepochs, a->cliprange, a->cliprange_vf};
            literal.quiet = true;
            PPO2& algo = a->reference_loop ? literal : algorithm;
            algo.seed = a->seed;
            if (x) algo.set_target_kl(x->target_kl);
            if (x) { algo.explicit_noise = x->noise; algo.explicit_perms = x->perms; }
            const auto t0 = std::chrono::steady_clock::now();
            algo.learn(a->n_updates * a->n_envs * a->n_steps);
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            const auto& hist = algo.history();
            if (hist.empty()) throw std::runtime_error("no update ran");
            // the first update pays allocation + graph capture, and the first env step after that capture pays a one-off
            // ~8 ms in the runtime: report the steady state (from the third update on) when there is one
            size_t from = hist.size() > 2 ? 2 : hist.size() > 1 ? 1 : 0;
            double c = 0, u = 0;
            for (size_t i = from; i < hist.size(); ++i) { c += hist[i].collect_ms; u += hist[i].update_ms; }
            const double n = (double)(hist.size() - from);
            out->collect_ms = c / n; out->update_ms = u / n;
            out->env_steps_per_s = (double)a->n_envs * a->n_steps / ((c + u) / n / 1e3);
            std::memcpy(out->losses, hist.back().losses, sizeof out->losses);
            out->fps_last = hist.back().fps;
            (void)sec;
            out->phase_env_ms = algo.phase_env_ms / n; out->phase_act_ms = algo.phase_act_ms / n; out->phase_observe_ms = algo.phase_observe_ms / n;
            if (pool) { out->pool_workers = pool->pool_workers(); out->pool_chunk = pool->pool_chunk(); out->pool_active = pool->pool_active(); }
            nlohmann::json j;                                   // serialise round trip of the normaliser
            env.serialize(j);
            out->obs_count = j["obs_rms"]["count"].get<double>(); out->ret_count = j["ret_rms"]["count"].get<double>();
            env.deserialize(j);
            if (x) {
                if (x->losses_out) for (size_t i = 0; i < hist.size(); ++i) std::memcpy(x->losses_out + 5 * i, hist[i].losses, sizeof(float) * 5);
                if (x->reward_curve) for (size_t i = 0; i < hist.size(); ++i) x->reward_curve[i] = hist[i].mean_reward;
                if (x->applied_out) for (size_t i = 0; i < hist.size(); ++i) { x->applied_out[2 * i] = hist[i].applied; x->applied_out[2 * i + 1] = hist[i].total; }
                if (x->theta_out && ppo_get_flat(h, 0, x->theta_out, ppo_num_params(h)) != 0) throw std::runtime_error(ppo_last_error(h));
                if (x->obs_mean && ppo_norm_get_stats(h, 0, x->obs_mean, x->obs_var, x->obs_count) != 0) throw std::runtime_error(ppo_last_error(h));
                if (x->ret_mean && ppo_norm_get_stats(h, 1, x->ret_mean, x->ret_var, x->ret_count) != 0) throw std::runtime_error(ppo_last_error(h));
                if (x->count_names && x->counts && x->n_counts) {
                    int64_t c64[64];
                    const int nc = ppo_kernel_counts(h, 64, x->count_names, c64);
                    for (int i = 0; i < nc; ++i) x->counts[i] = (long long)c64[i];
                    *x->n_counts = nc;
                }
            }
        }
        ppo_destroy(h);
        return 0;
    } catch (const std::exception& e) {
        std::snprintf(out->error, sizeof out->error, "%s", e.what());
        if (h) ppo_destroy(h);
        return -1;
    }
}

int ppo_host_learn(const ppo_host_args* a, ppo_host_result* out) { return run_learn(a, out, nullptr); }

// PPO2::save of a categorical policy (a [64,64] handle behind DiscreteTargetEnv x 4 + EnvNormalize, one short learn()) under `prefix`, then PPO2::load into a
// FRESH categorical handle: every tensor and the deterministic actions of `n` observations must be identical (actions_out [2][n]: before / after), and
// loading into a Gaussian handle must fail.  Returns 0; 1 = tensors differ, 2 = the Gaussian load went through; -1 = error (message on stderr).
int ppo_host_discrete_checkpoint(const char* prefix, const float* obs, int n, float* actions_out) {
    ppo_handle* h[3] = {nullptr, nullptr, nullptr};
    int rc = 0;
    try {
        ppo_config cfg; const int32_t hidden[2] = {64, 64};
        ppo_config_default(&cfg, 18, 6, 2, hidden);
        for (int k = 0; k < 3; ++k)
            if (ppo_create_ex(&cfg, k < 2 ? PPO_ACT_CATEGORICAL : PPO_ACT_GAUSSIAN, &h[k]) != 0 || ppo_init_orthogonal(h[k], (uint64_t)k) != 0)
                throw std::runtime_error(ppo_last_error(h[k]));
        std::vector<std::shared_ptr<Env>> envs;
        for (uint32_t i = 0; i < 4; ++i) envs.push_back(std::make_shared<DiscreteTargetEnv>(1234u, i, 18, 6));
        {
            EnvNormalize env{std::unique_ptr<Env>(new VecEnv(envs, 1)), h[0], /*training=*/true};
            PPO2 algo{h[0], env, 0.99f, 16, cfg.ent_coef, 1e-3f, 0.5f, 0.5f, 0.95f, 4, 2, 0.2f};
            algo.quiet = true;
            algo.learn(2 * 4 * 16);
            algo.save(prefix);
            if (ppo_act_deterministic(h[0], obs, n, actions_out) != 0) throw std::runtime_error(ppo_last_error(h[0]));
        }
        {
            EnvNormalize env{std::unique_ptr<Env>(new DiscreteTargetEnv(1234u, 0, 18, 6)), h[1], /*training=*/false};
            PPO2 algo{h[1], env};
            algo.load(prefix);
            if (ppo_act_deterministic(h[1], obs, n, actions_out + n) != 0) throw std::runtime_error(ppo_last_error(h[1]));
        }
        for (int i = 0; i < ppo_num_tensors(h[0]) && !rc; ++i) {
            int32_t r = 0, c = 0;
            ppo_tensor_info(h[0], i, nullptr, &r, &c);
            std::vector<float> x((size_t)r * (c ? c : 1)), y(x.size());
            if (ppo_get_tensor(h[0], 0, i, x.data(), (int64_t)x.size()) != 0 || ppo_get_tensor(h[1], 0, i, y.data(), (int64_t)y.size()) != 0) throw std::runtime_error(ppo_last_error(h[1]));
            if (std::memcmp(x.data(), y.data(), sizeof(float) * x.size()) != 0) rc = 1;
        }
        if (!rc) {
            EnvNormalize env{std::unique_ptr<Env>(new EnvMock()), h[2], /*training=*/false};     // (SPACE_CONTINOUS, for the Gaussian handle)
            PPO2 algo{h[2], env};
            bool threw = false;
            try { algo.load(prefix); } catch (const std::exception& e) { threw = true; std::fprintf(stderr, "expected: %s\n", e.what()); }
            if (!threw) rc = 2;
        }
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); rc = -1; }
    for (ppo_handle* x : h) if (x) ppo_destroy(x);
    return rc;
}

// The learning check of the multi-categorical head (tests/test_multi_discrete.py): n_envs x MultiDiscreteTargetEnv(nvec) -> VecEnv -> EnvNormalize -> PPO2::learn with the
// library's own sampling and shuffles, through the HBM-resident loop or, with args->reference_loop, the literal one.  The handle comes from PPO2::create_handle (the Env
// carries IMultiDiscrete: ppo_create_multi_ex, with PPO_ACT_SHAPE_KERNELS when args->discrete_kernels == 1, with PPO_ACT_PAIR_KERNELS when it is 2, with PPO_ACT_BF16_MULTI_HEAD when args->compute_dtype is PPO_BF16).  args as for ppo_host_learn_masked plus n_components / nvec / multi_masked (the environments also carry IActionMask: PPO2 masks
// by itself).  reward_curve [n_updates]; *forbidden_received: steps on which an environment was sent a forbidden action; playback_actions [n_playback][K] /
// playback_legal [n_playback] (may be null / 0): PPO2::eval on the stack for n_playback steps after training (environment 0's row) and whether the environment's own mask
// allowed every component's action.  count_names / counts / n_counts (all three or none): ppo_kernel_counts of the run's handle, up to 64 entries.
int ppo_host_learn_multi(const ppo_host_args* a, float* reward_curve, long long* forbidden_received, int n_playback, float* playback_actions, float* playback_legal,
                         char (*count_names)[32], long long* counts, int* n_counts, ppo_host_result* out) {
    std::memset(out, 0, sizeof *out);
    ppo_handle* h = nullptr;
    try {
        if (a->n_components < 1 || a->n_components > 16) throw std::runtime_error("n_components must be 1..16");
        const std::vector<int> nvec(a->nvec, a->nvec + a->n_components);
        const int K = a->n_components, O = a->obs_dim > 0 ? a->obs_dim : 18;
        int A = 0;
        for (int n : nvec) A += n;
        ppo_config cfg;
        ppo_config_default(&cfg, O, A, a->n_hidden, a->hidden);
        cfg.device = a->device;
        cfg.compute_dtype = a->compute_dtype;
        std::vector<std::shared_ptr<MultiDiscreteTargetEnv>> kids;
        std::vector<std::shared_ptr<Env>> envs;
        for (int i = 0; i < a->n_envs; ++i) { kids.push_back(std::make_shared<MultiDiscreteTargetEnv>(1234u, (uint32_t)i, O, nvec, 100, a->multi_masked != 0)); envs.push_back(kids.back()); }
        // (PPO_BF16: the bf16 path's multi-categorical head is opt-in, as PPO_ACT_BF16_HEAD is for a discrete Env's handle)
        const int32_t extra_flags = (a->discrete_kernels == 2 ? PPO_ACT_PAIR_KERNELS : 0) | (a->compute_dtype == PPO_BF16 ? PPO_ACT_BF16_MULTI_HEAD : 0);
        if (PPO2::create_handle(cfg, *envs[0], &h, a->discrete_kernels == 1, extra_flags) != 0) throw std::runtime_error(ppo_last_error(nullptr));
        if (ppo_init_orthogonal(h, 0) != 0) throw std::runtime_error(ppo_last_error(h));
        if (a->host_step_fused && ppo_set_host_step_fused(h, 1) != 0) throw std::runtime_error(ppo_last_error(h));
        if (g_rollout_resident && ppo_set_rollout_resident(h, 1) != 0) throw std::runtime_error(ppo_last_error(h));
        {
            EnvNormalize env{std::unique_ptr<Env>(new VecEnv(envs, a->max_workers)), h, /*training=*/true, a->norm_obs != 0, a->norm_reward != 0, 10.f, 10.f, a->gamma};
            struct Plain : Env, IActionMask, IMultiDiscrete {       // hides the EnvNormalize type to force the reference loop; the two mixins stay visible
                EnvNormalize& e; explicit Plain(EnvNormalize& x) : e(x) {}
                std::string get_action_space() override { return e.get_action_space(); }
                std::string get_observation_space() override { return e.get_observation_space(); }
                int get_action_space_size() override { return e.get_action_space_size(); }
                int get_observation_space_size() override { return e.get_observation_space_size(); }
                int get_num_envs() override { return e.get_num_envs(); }
                Mat reset() override { return e.reset(); }
                std::vector<Mat> step(const Mat& x) override { return e.step(x); }
                void render() override {}
                float get_time() override { return 0; }
                Mat get_original_obs() override { return e.get_original_obs(); }
                Mat get_original_rew() override { return e.get_original_rew(); }
                void serialize(nlohmann::json& j) override { e.serialize(j); }
                void deserialize(nlohmann::json& j) override { e.deserialize(j); }
                Mat get_action_mask() override { return e.get_action_mask(); }
                bool has_action_mask() override { return e.has_action_mask(); }
                std::vector<int> get_action_nvec() override { return e.get_action_nvec(); }
                bool has_action_nvec() override { return e.has_action_nvec(); }
            } plain{env};
            Env& top = a->reference_loop ? static_cast<Env&>(plain) : static_cast<Env&>(env);
            PPO2 algo{h, top, a->gamma, a->n_steps, cfg.ent_coef, a->lr, 0.5f, 0.5f, a->lam, a->nminibatches, a->noptepochs, a->cliprange, a->cliprange_vf};
            if (ppo_get_action_masking(h) != (a->multi_masked ? 1 : 0)) throw std::runtime_error("PPO2 set action masking wrongly for this Env");
            algo.quiet = true;
            algo.seed = a->seed;
            algo.learn(a->n_updates * a->n_envs * a->n_steps);
            const auto& hist = algo.history();
            if (hist.empty()) throw std::runtime_error("no update ran");
            std::memcpy(out->losses, hist.back().losses, sizeof out->losses);
            out->fps_last = hist.back().fps;
            if (reward_curve) for (size_t i = 0; i < hist.size(); ++i) reward_curve[i] = hist[i].mean_reward;
            long long total = 0;
            for (const auto& k : kids) total += k->forbidden_received();
            if (forbidden_received) *forbidden_received = total;
            Mat obs = top.reset();
            for (int t = 0; t < n_playback; ++t) {
                const Mat mask = env.get_action_mask();
                const Mat act = algo.eval(obs);
                if (act.cols() != K) throw std::runtime_error("PPO2::eval did not return K action columns");
                bool legal = true;
                for (int k = 0, o = 0; k < K; o += nvec[k], ++k) {
                    const int c = (int)act(0, k);
                    if (playback_actions) playback_actions[(size_t)t * K + k] = act(0, k);
                    legal = legal && c >= 0 && c < nvec[k] && mask(0, o + c) != 0.f;
                }
                if (playback_legal) playback_legal[t] = legal ? 1.f : 0.f;
                obs = top.step(act)[0];
            }
            if (count_names && counts && n_counts) {
                int64_t c64[64];
                const int nc = ppo_kernel_counts(h, 64, count_names, c64);
                for (int i = 0; i < nc; ++i) counts[i] = (long long)c64[i];
                *n_counts = nc;
            }
        }
        ppo_destroy(h);
        return 0;
    } catch (const std::exception& e) {
        std::snprintf(out->error, sizeof out->error, "%s", e.what());
        if (h) ppo_destroy(h);
        return -1;
    }
}

// PPO2::save of a multi-categorical policy (a [64,64] handle with components nvec behind MultiDiscreteTargetEnv x 4 + EnvNormalize, one short learn()) under `prefix`,
// then PPO2::load into a FRESH handle with the same components: every tensor and the deterministic actions of `n` observations must be identical (actions_out
// [2][n][K]: before / after).  Loading into a handle with ANOTHER split of the same width (other_nvec, same sum) and into a plain categorical handle of that width must
// both fail.  Returns 0; 1 = tensors differ, 2 = the other split's load went through, 3 = the categorical handle's; -1 = error (message on stderr).
int ppo_host_multi_checkpoint(const char* prefix, const int* nvec_in, const int* other_nvec_in, int K, int K_other, const float* obs, int n, float* actions_out) {
    ppo_handle* h[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = 0;
    try {
        const std::vector<int> nvec(nvec_in, nvec_in + K), other(other_nvec_in, other_nvec_in + K_other);
        int A = 0;
        for (int x : nvec) A += x;
        ppo_config cfg; const int32_t hidden[2] = {64, 64};
        ppo_config_default(&cfg, 18, A, 2, hidden);
        MultiDiscreteTargetEnv probe(1234u, 0, 18, nvec), probe_other(1234u, 0, 18, other);
        DiscreteTargetEnv probe_cat(1234u, 0, 18, A);
        Env* probes[4] = {&probe, &probe, &probe_other, &probe_cat};
        for (int k = 0; k < 4; ++k)
            if (PPO2::create_handle(cfg, *probes[k], &h[k]) != 0 || ppo_init_orthogonal(h[k], (uint64_t)k) != 0) throw std::runtime_error(ppo_last_error(h[k]));
        std::vector<std::shared_ptr<Env>> envs;
        for (uint32_t i = 0; i < 4; ++i) envs.push_back(std::make_shared<MultiDiscreteTargetEnv>(1234u, i, 18, nvec));
        {
            EnvNormalize env{std::unique_ptr<Env>(new VecEnv(envs, 1)), h[0], /*training=*/true};
            PPO2 algo{h[0], env, 0.99f, 16, cfg.ent_coef, 1e-3f, 0.5f, 0.5f, 0.95f, 4, 2, 0.2f};
            algo.quiet = true;
            algo.learn(2 * 4 * 16);
            algo.save(prefix);
            if (ppo_act_deterministic(h[0], obs, n, actions_out) != 0) throw std::runtime_error(ppo_last_error(h[0]));
        }
        {
            EnvNormalize env{std::unique_ptr<Env>(new MultiDiscreteTargetEnv(1234u, 0, 18, nvec)), h[1], /*training=*/false};
            PPO2 algo{h[1], env};
            algo.load(prefix);
            if (ppo_act_deterministic(h[1], obs, n, actions_out + (size_t)n * K) != 0) throw std::runtime_error(ppo_last_error(h[1]));
        }
        for (int i = 0; i < ppo_num_tensors(h[0]) && !rc; ++i) {
            int32_t r = 0, c = 0;
            ppo_tensor_info(h[0], i, nullptr, &r, &c);
            std::vector<float> x((size_t)r * (c ? c : 1)), y(x.size());
            if (ppo_get_tensor(h[0], 0, i, x.data(), (int64_t)x.size()) != 0 || ppo_get_tensor(h[1], 0, i, y.data(), (int64_t)y.size()) != 0) throw std::runtime_error(ppo_last_error(h[1]));
            if (std::memcmp(x.data(), y.data(), sizeof(float) * x.size()) != 0) rc = 1;
        }
        for (int k = 2; k < 4 && !rc; ++k) {
            std::unique_ptr<Env> e(k == 2 ? static_cast<Env*>(new MultiDiscreteTargetEnv(1234u, 0, 18, other)) : static_cast<Env*>(new DiscreteTargetEnv(1234u, 0, 18, A)));
            EnvNormalize env{std::move(e), h[k], /*training=*/false};
            PPO2 algo{h[k], env};
            bool threw = false;
            try { algo.load(prefix); } catch (const std::exception& ex) { threw = true; std::fprintf(stderr, "expected: %s\n", ex.what()); }
            if (!threw) rc = k;
        }
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); rc = -1; }
    for (ppo_handle* x : h) if (x) ppo_destroy(x);
    return rc;
}

// The learning check of the multi-binary head (tests/test_multi_binary.py): n_envs x MultiBinaryTargetEnv(act_dim bits) -> VecEnv -> EnvNormalize -> PPO2::learn with the
// library's own sampling and shuffles, through the HBM-resident loop or, with args->reference_loop, the literal one.  The handle comes from PPO2::create_handle (the Env
// carries IMultiBinary: ppo_create_ex with PPO_ACT_MULTI_BINARY; args->discrete_kernels == 3 adds PPO_ACT_BINARY_SHAPE_KERNELS -- the narrow <mbin> kernels where
// the shape qualifies -- 4 adds PPO_ACT_BINARY_PAIR_KERNELS -- the [256,256] train kernel pair where that shape qualifies -- 1 and 2 ask for the flags of a discrete Env's handle, which this head accepts and ignores).  The head has neither a fused host step nor a resident rollout: args->host_step_fused and the process-wide resident default are not applied.
// reward_curve [n_updates], losses_out [n_updates][5] (may be null); count_names / counts / n_counts (all three or none): every kernel variant of the
// run's handle (ppo_kernel_variant_name / ppo_kernel_count: the list grows between versions), up to 64 entries.
int ppo_host_learn_binary(const ppo_host_args* a, float* reward_curve, float* losses_out, char (*count_names)[32], long long* counts, int* n_counts, ppo_host_result* out) {
    std::memset(out, 0, sizeof *out);
    ppo_handle* h = nullptr;
    try {
        const int O = a->obs_dim > 0 ? a->obs_dim : 18, A = a->act_dim > 0 ? a->act_dim : 18;
        ppo_config cfg;
        ppo_config_default(&cfg, O, A, a->n_hidden, a->hidden);
        cfg.device = a->device;
        cfg.compute_dtype = a->compute_dtype;
        std::vector<std::shared_ptr<Env>> envs;
        for (int i = 0; i < a->n_envs; ++i) envs.push_back(std::make_shared<MultiBinaryTargetEnv>(1234u, (uint32_t)i, O, A));
        const int32_t extra_flags = a->discrete_kernels == 2 ? PPO_ACT_PAIR_KERNELS : a->discrete_kernels == 3 ? PPO_ACT_BINARY_SHAPE_KERNELS : a->discrete_kernels == 4 ? PPO_ACT_BINARY_PAIR_KERNELS : 0;
        if (PPO2::create_handle(cfg, *envs[0], &h, a->discrete_kernels == 1, extra_flags) != 0) throw std::runtime_error(ppo_last_error(nullptr));
        if (ppo_action_dist(h) != PPO_ACT_MULTI_BINARY) throw std::runtime_error("PPO2::create_handle did not create a multi-binary handle for an IMultiBinary Env");
        if (ppo_init_orthogonal(h, 0) != 0) throw std::runtime_error(ppo_last_error(h));
        {
            EnvNormalize env{std::unique_ptr<Env>(new VecEnv(envs, a->max_workers)), h, /*training=*/true, a->norm_obs != 0, a->norm_reward != 0, 10.f, 10.f, a->gamma};
            struct Plain : Env, IMultiBinary {       // hides the EnvNormalize type to force the reference loop; the mixin stays visible
                EnvNormalize& e; explicit Plain(EnvNormalize& x) : e(x) {}
                std::string get_action_space() override { return e.get_action_space(); }
                std::string get_observation_space() override { return e.get_observation_space(); }
                int get_action_space_size() override { return e.get_action_space_size(); }
                int get_observation_space_size() override { return e.get_observation_space_size(); }
                int get_num_envs() override { return e.get_num_envs(); }
                Mat reset() override { return e.reset(); }
                std::vector<Mat> step(const Mat& x) override { return e.step(x); }
                void render() override {}
                float get_time() override { return 0; }
                Mat get_original_obs() override { return e.get_original_obs(); }
                Mat get_original_rew() override { return e.get_original_rew(); }
                void serialize(nlohmann::json& j) override { e.serialize(j); }
                void deserialize(nlohmann::json& j) override { e.deserialize(j); }
                bool has_binary_actions() override { return e.has_binary_actions(); }
            } plain{env};
            Env& top = a->reference_loop ? static_cast<Env&>(plain) : static_cast<Env&>(env);
            PPO2 algo{h, top, a->gamma, a->n_steps, cfg.ent_coef, a->lr, 0.5f, 0.5f, a->lam, a->nminibatches, a->noptepochs, a->cliprange, a->cliprange_vf};
            if (ppo_get_action_masking(h) != 0) throw std::runtime_error("PPO2 set action masking for a multi-binary Env");
            algo.quiet = true;
            algo.seed = a->seed;
            algo.learn(a->n_updates * a->n_envs * a->n_steps);
            const auto& hist = algo.history();
            if (hist.empty()) throw std::runtime_error("no update ran");
            std::memcpy(out->losses, hist.back().losses, sizeof out->losses);
            out->fps_last = hist.back().fps;
            if (reward_curve) for (size_t i = 0; i < hist.size(); ++i) reward_curve[i] = hist[i].mean_reward;
            if (losses_out) for (size_t i = 0; i < hist.size(); ++i) std::memcpy(losses_out + 5 * i, hist[i].losses, sizeof(float) * 5);
            if (count_names && counts && n_counts) {
                int nc = 0;
                for (const char* nm; nc < 64 && (nm = ppo_kernel_variant_name(nc)) != nullptr; ++nc) {
                    std::snprintf(count_names[nc], 32, "%s", nm);
                    counts[nc] = (long long)ppo_kernel_count(h, nm);
                }
                *n_counts = nc;
            }
        }
        ppo_destroy(h);
        return 0;
    } catch (const std::exception& e) {
        std::snprintf(out->error, sizeof out->error, "%s", e.what());
        if (h) ppo_destroy(h);
        return -1;
    }
}

// PPO2::save of a multi-binary policy (a [64,64] handle of 6 bits behind MultiBinaryTargetEnv x 4 + EnvNormalize, one short learn()) under `prefix`, then PPO2::load into
// a FRESH multi-binary handle: every tensor and the deterministic actions of `n` observations must be identical (actions_out [2][n][6]: before / after).  Loading it
// into a categorical handle of the same width must fail, and so must loading a categorical policy's checkpoint (written under <prefix>.cat) into the multi-binary
// handle.  Returns 0; 1 = tensors differ, 2 = the categorical handle's load went through, 3 = the multi-binary handle's load of the categorical checkpoint; -1 = error
// (message on stderr).  discrete_kernels == 3 (ppo_host_args::discrete_kernels' "binary narrow"): both multi-binary handles are created with
// PPO_ACT_BINARY_SHAPE_KERNELS; 4 ("binary pair"): with PPO_ACT_BINARY_PAIR_KERNELS, and every handle has hidden [256,256], the shape on which that flag takes
// effect; any other value: without.
int ppo_host_binary_checkpoint_ex(const char* prefix, const float* obs, int n, float* actions_out, int discrete_kernels) {
    ppo_handle* h[3] = {nullptr, nullptr, nullptr};
    int rc = 0;
    try {
        const int A = 6;
        ppo_config cfg; const int32_t width = discrete_kernels == 4 ? 256 : 64, hidden[2] = {width, width};
        ppo_config_default(&cfg, 18, A, 2, hidden);
        const int32_t binary_flags = discrete_kernels == 3 ? PPO_ACT_BINARY_SHAPE_KERNELS : discrete_kernels == 4 ? PPO_ACT_BINARY_PAIR_KERNELS : 0;
        MultiBinaryTargetEnv probe(1234u, 0, 18, A);
        DiscreteTargetEnv probe_cat(1234u, 0, 18, A);
        Env* probes[3] = {&probe, &probe, &probe_cat};
        for (int k = 0; k < 3; ++k)
            if (PPO2::create_handle(cfg, *probes[k], &h[k], false, k < 2 ? binary_flags : 0) != 0 || ppo_init_orthogonal(h[k], (uint64_t)k) != 0) throw std::runtime_error(ppo_last_error(h[k]));
        std::vector<std::shared_ptr<Env>> envs;
        for (uint32_t i = 0; i < 4; ++i) envs.push_back(std::make_shared<MultiBinaryTargetEnv>(1234u, i, 18, A));
        {
            EnvNormalize env{std::unique_ptr<Env>(new VecEnv(envs, 1)), h[0], /*training=*/true};
            PPO2 algo{h[0], env, 0.99f, 16, cfg.ent_coef, 1e-3f, 0.5f, 0.5f, 0.95f, 4, 2, 0.2f};
            algo.quiet = true;
            algo.learn(2 * 4 * 16);
            algo.save(prefix);
            if (ppo_act_deterministic(h[0], obs, n, actions_out) != 0) throw std::runtime_error(ppo_last_error(h[0]));
        }
        {
            EnvNormalize env{std::unique_ptr<Env>(new MultiBinaryTargetEnv(1234u, 0, 18, A)), h[1], /*training=*/false};
            PPO2 algo{h[1], env};
            algo.load(prefix);
            if (ppo_act_deterministic(h[1], obs, n, actions_out + (size_t)n * A) != 0) throw std::runtime_error(ppo_last_error(h[1]));
        }
        for (int i = 0; i < ppo_num_tensors(h[0]) && !rc; ++i) {
            int32_t r = 0, c = 0;
            ppo_tensor_info(h[0], i, nullptr, &r, &c);
            std::vector<float> x((size_t)r * (c ? c : 1)), y(x.size());
            if (ppo_get_tensor(h[0], 0, i, x.data(), (int64_t)x.size()) != 0 || ppo_get_tensor(h[1], 0, i, y.data(), (int64_t)y.size()) != 0) throw std::runtime_error(ppo_last_error(h[1]));
            if (std::memcmp(x.data(), y.data(), sizeof(float) * x.size()) != 0) rc = 1;
        }
        if (!rc) {
            EnvNormalize env{std::unique_ptr<Env>(new DiscreteTargetEnv(1234u, 0, 18, A)), h[2], /*training=*/false};
            PPO2 algo{h[2], env};
            bool threw = false;
            try { algo.load(prefix); } catch (const std::exception& ex) { threw = true; std::fprintf(stderr, "expected: %s\n", ex.what()); }
            if (!threw) rc = 2;
            algo.save(std::string(prefix) + ".cat");
        }
        if (!rc) {
            EnvNormalize env{std::unique_ptr<Env>(new MultiBinaryTargetEnv(1234u, 0, 18, A)), h[1], /*training=*/false};
            PPO2 algo{h[1], env};
            bool threw = false;
            try { algo.load(std::string(prefix) + ".cat"); } catch (const std::exception& ex) { threw = true; std::fprintf(stderr, "expected: %s\n", ex.what()); }
            if (!threw) rc = 3;
        }
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); rc = -1; }
    for (ppo_handle* x : h) if (x) ppo_destroy(x);
    return rc;
}
int ppo_host_binary_checkpoint(const char* prefix, const float* obs, int n, float* actions_out) { return ppo_host_binary_checkpoint_ex(prefix, obs, n, actions_out, 0); }

// PPO2::learn with EXPLICIT exploration noise and epoch permutations on the reference's stack (SeededEnvMock x N -> VecEnv ->
// EnvNormalize -> PPO2; ppo2.cpp:188-250), through the HBM-resident loop or (reference_loop) the literal one: what
// tests/test_host_layer.py holds against oracle.collect + oracle.update update by update (ppo2.hpp:264-349).
int ppo_host_learn_explicit(const ppo_host_args* a, const ppo_host_explicit* x, ppo_host_result* out) { return run_learn(a, out, x); }

// The learning check of the time-limit bootstrap (tests/test_truncation.py): n_envs x TimeLimit(UnitRewardEnv, time_limit) -> VecEnv -> EnvNormalize -> PPO2::learn
// through the HBM-resident loop with the library's own sampling and shuffles (args: n_envs, n_steps, hidden, nminibatches, noptepochs, n_updates, lr, cliprange,
// gamma, lam, norm_obs, norm_reward, seed, obs_dim, act_dim, cliprange_vf, device; the rest is ignored).  bootstrap = PPO2::bootstrap_truncated.  Afterwards the
// critic is read on `probe_raw` [n_probe, O] (n_probe a multiple of n_envs), scaled with the final observation statistics: probe_values [n_probe].
// time_limit <= 0: no wrapper (the environment never ends an episode).  losses_out [n_updates][5] may be null.
int ppo_host_learn_time_limit(const ppo_host_args* a, int time_limit, int bootstrap, const float* probe_raw, int n_probe, float* probe_values, float* losses_out,
                              ppo_host_result* out) {
    std::memset(out, 0, sizeof *out);
    ppo_handle* h = nullptr;
    try {
        ppo_config cfg;
        const int O = a->obs_dim > 0 ? a->obs_dim : 18, A = a->act_dim > 0 ? a->act_dim : 18;
        if (n_probe < 0 || n_probe % a->n_envs != 0) throw std::runtime_error("n_probe must be a multiple of n_envs");
        ppo_config_default(&cfg, O, A, a->n_hidden, a->hidden);
        cfg.device = a->device;
        if (ppo_create(&cfg, &h) != 0) throw std::runtime_error(ppo_last_error(nullptr));
        if (ppo_init_orthogonal(h, a->seed) != 0) throw std::runtime_error(ppo_last_error(h));
        std::vector<std::shared_ptr<Env>> envs;
        for (int i = 0; i < a->n_envs; ++i) {
            std::shared_ptr<Env> e = std::make_shared<UnitRewardEnv>(1234u, (uint32_t)i, O, A);
            envs.push_back(time_limit > 0 ? std::shared_ptr<Env>(std::make_shared<TimeLimit>(e, time_limit)) : e);
        }
        {
            std::unique_ptr<Env> inner;
            if (a->n_envs > 1) inner.reset(new VecEnv(envs, a->max_workers));
            else inner.reset(time_limit > 0 ? static_cast<Env*>(new TimeLimit(std::make_shared<UnitRewardEnv>(1234u, 0u, O, A), time_limit)) : static_cast<Env*>(new UnitRewardEnv(1234u, 0u, O, A)));
            EnvNormalize env{std::move(inner), h, /*training=*/true, a->norm_obs != 0, a->norm_reward != 0, 10.f, 10.f, a->gamma};
            PPO2 algo{h, env, a->gamma, a->n_steps, cfg.ent_coef, a->lr, 0.5f, 0.5f, a->lam, a->nminibatches, a->noptepochs, a->cliprange, a->cliprange_vf};
            algo.quiet = true;
            algo.seed = a->seed;
            algo.bootstrap_truncated = bootstrap != 0;
            algo.learn(a->n_updates * a->n_envs * a->n_steps);
            const auto& hist = algo.history();
            if (hist.empty()) throw std::runtime_error("no update ran");
            std::memcpy(out->losses, hist.back().losses, sizeof out->losses);
            out->fps_last = hist.back().fps;
            if (losses_out) for (size_t i = 0; i < hist.size(); ++i) std::memcpy(losses_out + 5 * i, hist[i].losses, sizeof(float) * 5);
            for (int r0 = 0; r0 < n_probe; r0 += a->n_envs) {
                Mat raw(a->n_envs, O);
                std::memcpy(raw.data(), probe_raw + (size_t)r0 * O, sizeof(float) * (size_t)a->n_envs * O);
                const Mat x = env.normalize_terminal(raw);
                if (ppo_value(h, x.data(), a->n_envs, probe_values + r0) != 0) throw std::runtime_error(ppo_last_error(h));
            }
        }
        ppo_destroy(h);
        return 0;
    } catch (const std::exception& e) {
        std::snprintf(out->error, sizeof out->error, "%s", e.what());
        if (h) ppo_destroy(h);
        return -1;
    }
}

// The learning check of action masks (tests/test_action_mask.py): n_envs x MaskedTargetEnv -> VecEnv -> EnvNormalize -> PPO2::learn with the library's own sampling and
// shuffles, through the HBM-resident loop (ppo_rollout_act_masked) or, with args->reference_loop, the literal one (ppo_step_masked / ppo_train_step_masked).  args: n_envs,
// n_steps, hidden, nminibatches, noptepochs, n_updates, lr, cliprange, gamma, lam, norm_obs, norm_reward, seed, obs_dim, act_dim (categories), cliprange_vf, device,
// max_workers, reference_loop.  reward_curve [n_updates]: mean un-normalised reward of every update's rollout; *forbidden_received: forbidden actions the environments
// were sent over the whole run (a masking policy sends none); playback_actions / playback_legal [n_playback] (may be null / 0): PPO2::eval on environment 0's
// stack for n_playback steps after training, and whether the environment's own mask allowed each action.
int ppo_host_learn_masked(const ppo_host_args* a, float* reward_curve, long long* forbidden_received, int n_playback, float* playback_actions, float* playback_legal,
                          ppo_host_result* out) {
    std::memset(out, 0, sizeof *out);
    ppo_handle* h = nullptr;
    try {
        ppo_config cfg;
        const int O = a->obs_dim > 0 ? a->obs_dim : 18, A = a->act_dim > 0 ? a->act_dim : 18;
        ppo_config_default(&cfg, O, A, a->n_hidden, a->hidden);
        cfg.device = a->device;
        { MaskedTargetEnv probe(1234u, 0, O, A);
          cfg.compute_dtype = a->compute_dtype;
          if (ppo_create_ex(&cfg, host_action_dist(probe, a), &h) != 0) throw std::runtime_error(ppo_last_error(nullptr)); }
        if (ppo_init_orthogonal(h, 0) != 0) throw std::runtime_error(ppo_last_error(h));
        if (a->host_step_fused && ppo_set_host_step_fused(h, 1) != 0) throw std::runtime_error(ppo_last_error(h));
        if (g_rollout_resident && ppo_set_rollout_resident(h, 1) != 0) throw std::runtime_error(ppo_last_error(h));
        std::vector<std::shared_ptr<MaskedTargetEnv>> kids;
        std::vector<std::shared_ptr<Env>> envs;
        for (int i = 0; i < a->n_envs; ++i) { kids.push_back(std::make_shared<MaskedTargetEnv>(1234u, (uint32_t)i, O, A)); envs.push_back(kids.back()); }
        {
            EnvNormalize env{std::unique_ptr<Env>(new VecEnv(envs, a->max_workers)), h, /*training=*/true, a->norm_obs != 0, a->norm_reward != 0, 10.f, 10.f, a->gamma};
            struct Plain : Env, IActionMask {       // hides the EnvNormalize type to force the reference loop; the mask mixin stays visible
                EnvNormalize& e; explicit Plain(EnvNormalize& x) : e(x) {}
                std::string get_action_space() override { return e.get_action_space(); }
                std::string get_observation_space() override { return e.get_observation_space(); }
                int get_action_space_size() override { return e.get_action_space_size(); }
                int get_observation_space_size() override { return e.get_observation_space_size(); }
                int get_num_envs() override { return e.get_num_envs(); }
                Mat reset() override { return e.reset(); }
                std::vector<Mat> step(const Mat& x) override { return e.step(x); }
                void render() override {}
                float get_time() override { return 0; }
                Mat get_original_obs() override { return e.get_original_obs(); }
                Mat get_original_rew() override { return e.get_original_rew(); }
                void serialize(nlohmann::json& j) override { e.serialize(j); }
                void deserialize(nlohmann::json& j) override { e.deserialize(j); }
                Mat get_action_mask() override { return e.get_action_mask(); }
                bool has_action_mask() override { return e.has_action_mask(); }
            } plain{env};
            Env& top = a->reference_loop ? static_cast<Env&>(plain) : static_cast<Env&>(env);
            PPO2 algo{h, top, a->gamma, a->n_steps, cfg.ent_coef, a->lr, 0.5f, 0.5f, a->lam, a->nminibatches, a->noptepochs, a->cliprange, a->cliprange_vf};
            if (ppo_get_action_masking(h) != 1) throw std::runtime_error("PPO2 did not turn action masking on for an Env with the IActionMask mixin");
            algo.quiet = true;
            algo.seed = a->seed;
            algo.learn(a->n_updates * a->n_envs * a->n_steps);
            const auto& hist = algo.history();
            if (hist.empty()) throw std::runtime_error("no update ran");
            std::memcpy(out->losses, hist.back().losses, sizeof out->losses);
            out->fps_last = hist.back().fps;
            if (reward_curve) for (size_t i = 0; i < hist.size(); ++i) reward_curve[i] = hist[i].mean_reward;
            long long total = 0;
            for (const auto& k : kids) total += k->forbidden_received();
            if (forbidden_received) *forbidden_received = total;
            // playback: deterministic actions under the environments' masks (the statistics stay as training left them; EnvNormalize keeps updating them here, which the check does not mind)
            Mat obs = top.reset();
            for (int t = 0; t < n_playback; ++t) {
                const Mat mask = env.get_action_mask();
                const Mat act = algo.eval(obs);
                const int c = (int)act(0, 0);
                if (playback_actions) playback_actions[t] = act(0, 0);
                if (playback_legal) playback_legal[t] = c >= 0 && c < A && mask(0, c) != 0.f ? 1.f : 0.f;
                obs = top.step(act)[0];
            }
        }
        keep_kernel_counts(h);
        ppo_destroy(h);
        return 0;
    } catch (const std::exception& e) {
        std::snprintf(out->error, sizeof out->error, "%s", e.what());
        if (h) ppo_destroy(h);
        return -1;
    }
}

// PPO2::save of a [64,64] Gaussian policy built with `cliprange_vf` under `prefix` (no training), then PPO2::load into a FRESH handle behind a PPO2 built with the
// default -1: reports the value clipping that the load left on the fresh handle (ppo_get_value_clip).  Returns 0; -1 = error (message on stderr).
int ppo_host_value_clip_checkpoint(const char* prefix, float cliprange_vf, int32_t* mode, float* range) {
    ppo_handle* h[2] = {nullptr, nullptr};
    int rc = 0;
    try {
        ppo_config cfg; const int32_t hidden[2] = {64, 64};
        ppo_config_default(&cfg, 18, 18, 2, hidden);
        for (int k = 0; k < 2; ++k)
            if (ppo_create(&cfg, &h[k]) != 0 || ppo_init_orthogonal(h[k], (uint64_t)k) != 0) throw std::runtime_error(ppo_last_error(h[k]));
        {
            EnvNormalize env{std::unique_ptr<Env>(new EnvMock()), h[0], /*training=*/false};
            PPO2 algo{h[0], env, 0.99f, 16, cfg.ent_coef, 1e-3f, 0.5f, 0.5f, 0.95f, 4, 2, 0.2f, cliprange_vf};
            algo.save(prefix);
        }
        {
            EnvNormalize env{std::unique_ptr<Env>(new EnvMock()), h[1], /*training=*/false};
            PPO2 algo{h[1], env};
            algo.load(prefix);
            if (ppo_get_value_clip(h[1], mode, range) != 0) throw std::runtime_error(ppo_last_error(h[1]));
        }
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); rc = -1; }
    for (ppo_handle* x : h) if (x) ppo_destroy(x);
    return rc;
}

// PPO2::save of a [64,64] Gaussian policy with set_target_kl(target_kl) under `prefix` (no training), then PPO2::load into a FRESH handle: *loaded is that handle's
// ppo_get_target_kl.  strip_key: the "target_kl" key is first removed from the side-car -- a checkpoint from before the setting.  Returns 0; -1 = error (message on stderr).
int ppo_host_target_kl_checkpoint(const char* prefix, float target_kl, int strip_key, float* loaded) {
    ppo_handle* h[2] = {nullptr, nullptr};
    int rc = 0;
    try {
        ppo_config cfg; const int32_t hidden[2] = {64, 64};
        ppo_config_default(&cfg, 18, 18, 2, hidden);
        for (int k = 0; k < 2; ++k)
            if (ppo_create(&cfg, &h[k]) != 0 || ppo_init_orthogonal(h[k], (uint64_t)k) != 0) throw std::runtime_error(ppo_last_error(h[k]));
        {
            EnvNormalize env{std::unique_ptr<Env>(new EnvMock()), h[0], /*training=*/false};
            PPO2 algo{h[0], env};
            algo.set_target_kl(target_kl);
            algo.save(prefix);
        }
        if (strip_key) {
            const std::string path = std::string(prefix) + ".json";
            if (!nlohmann::json::parse(ckpt::slurp(path)).contains("target_kl")) throw std::runtime_error("the side-car has no target_kl key");
            // (the keys are written in sorted order: this one is neither the first nor the last)
            const std::string text = std::regex_replace(ckpt::slurp(path), std::regex("\"target_kl\"\\s*:\\s*[^,}]*,\\s*"), "");
            if (nlohmann::json::parse(text).contains("target_kl")) throw std::runtime_error("could not strip target_kl from the side-car");
            std::ofstream f(path);
            f << text;
        }
        {
            EnvNormalize env{std::unique_ptr<Env>(new EnvMock()), h[1], /*training=*/false};
            PPO2 algo{h[1], env};
            algo.set_target_kl(0.5f);                                 // (what load must overwrite)
            algo.load(prefix);
            if (ppo_get_target_kl(h[1], loaded) != 0) throw std::runtime_error(ppo_last_error(h[1]));
            if (algo.target_kl() != *loaded) throw std::runtime_error("PPO2::load left PPO2 and the handle with different target_kl");
        }
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); rc = -1; }
    for (ppo_handle* x : h) if (x) ppo_destroy(x);
    return rc;
}

// The policy queries of the host layer on a handle the CALLER owns (`handle` is a ppo_handle*; nothing is created or destroyed here): an MlpPolicy on it, then
// MlpPolicy::evaluate_actions -> values, neglogps, entropies [n]; MlpPolicy::proba_step -> params [n, ppo_distribution_width]; PPO2::action_probability with the
// actions -> prob [n] and, with logp, logprob [n].  obs [n, obs_dim], actions [n, ppo_action_width], mask [n, mask_cols] or null.  Returns 0; -1 = error (stderr).
int ppo_host_policy_query(void* handle, const float* obs, int obs_dim, const float* actions, const float* mask, int mask_cols, int n, float* values, float* neglogps,
                          float* entropies, float* params, float* prob, float* logprob) {
    try {
        ppo_handle* h = static_cast<ppo_handle*>(handle);
        MlpPolicy policy(h, 0);
        auto mat = [](const float* src, int rows, int cols) { Mat m(rows, cols); std::memcpy(m.data(), src, sizeof(float) * (size_t)rows * cols); return m; };
        auto put = [](const Mat& m, float* dst) { std::memcpy(dst, m.data(), sizeof(float) * (size_t)m.size()); };
        const Mat o = mat(obs, n, obs_dim), a = mat(actions, n, policy.action_width());
        Mat mk;
        if (mask) mk = mat(mask, n, mask_cols);
        const Mat* mp = mask ? &mk : nullptr;
        const std::vector<Mat> r = policy.evaluate_actions(o, a, mp);
        put(r[0], values); put(r[1], neglogps); put(r[2], entropies);
        put(policy.proba_step(o, mp), params);
        put(PPO2::action_probability(policy, o, &a, false, mp), prob);
        put(PPO2::action_probability(policy, o, &a, true, mp), logprob);
        return 0;
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return -1; }
}

// sizeof(ppo_host_args), sizeof(ppo_host_explicit): the Python mirrors check their layouts against these
int ppo_host_args_size(void) { return (int)sizeof(ppo_host_args); }
int ppo_host_explicit_size(void) { return (int)sizeof(ppo_host_explicit); }

}  // extern "C"
