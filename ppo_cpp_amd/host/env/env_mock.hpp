// env_mock.hpp -- test doubles behind the Env interface.
//   EnvMock        behaviour of the reference's stub (env/env_mock.hpp:18-92): 18 obs / 18 act, observation and reward
//                  are the constant scaling_coeff, done on every 300th call, actions ignored.
//   SeededEnvMock  same shape, non-degenerate data: obs ~ U(-1,1)^18, reward ~ U(-1,1), done ~ Bernoulli(1/300) from
//                  the counter hash keyed by (seed, env id, step) that the device-side synthetic env also uses.
//   TargetEnv      a LEARNABLE task on SeededEnvMock's observation stream: reward = -mean_j (a_j - (W obs)_j)^2 for a fixed hashed
//                  matrix W, episodes of a fixed length.  The reference's only validation is that it learns (README.md:22-24: the
//                  hexapod's reward curves); this is the environment behind tests/test_learning.py, small enough for the oracle.
//   DiscreteTargetEnv  the same on a DISCRETE action space (SPACE_DISCRETE, A categories; an action is [1,1] = the category index):
//                  reward 1 when a == argmax_j (W obs)_j with TargetEnv's W, 0 otherwise; episodes of a fixed length (tests/test_discrete_policy.py).
//   MaskedTargetEnv  DiscreteTargetEnv's task on the same W with state-dependent LEGALITY (the IActionMask mixin, action_mask.hpp): at every step a seeded subset of
//                  the categories (about half; keyed like the observations, columns obs_dim + j of the same stream) is forbidden, the target category never.
//                  Reward 1 for the target, 0 for another allowed category, -1 for a forbidden one; the environment counts the forbidden actions it received
//                  (tests/test_action_mask.py: a masking policy must never send one).
//   MultiDiscreteTargetEnv  DiscreteTargetEnv's task on a MULTI-DISCRETE action space (the IMultiDiscrete mixin, multi_discrete.hpp): K components of nvec[k] categories,
//                  an action is [1, K]; component k's target is argmax_j (W_k obs)_j with W_k hashed like TargetEnv's W under a per-component key; reward = the
//                  fraction of components whose action hits its target; episodes of a fixed length (tests/test_multi_discrete.py).  With masked = true it also
//                  carries IActionMask like MaskedTargetEnv: at every step a seeded subset (about half; the top bit of the stream's word (step, obs_dim + j) for
//                  global column j) of each component's categories is forbidden, the component's target never; the reward is -1 when any component's action is
//                  forbidden, and the environment counts the steps on which it received one.
//   MultiBinaryTargetEnv  the same on a MULTI-BINARY action space (the IMultiBinary mixin, multi_binary.hpp): A bits, an action is [1, A] of 0 / 1; bit j's target is
//                  (W obs)_j > 0 with TargetEnv's W; reward = the share of bits that hit their target, so a uniform policy earns 0.5; episodes of a fixed length
//                  (tests/test_multi_binary.py).
//   UnitRewardEnv  SeededEnvMock's observation stream, reward 1 on every step, never done by itself: behind a TimeLimit every episode ends by truncation, and
//                  the value of every state is 1 / (1 - gamma) -- which a critic only learns when the value is bootstrapped there (tests/test_truncation.py).
//                  reset() does NOT rewind the stream (it moves one draw on): no observation ever comes twice, so nothing tells a critic how far the
//                  episode has come, and the observation an episode ends on is a draw like any other.
#pragma once
#include <cstdint>

#include "action_mask.hpp"
#include "env.hpp"
#include "multi_binary.hpp"
#include "multi_discrete.hpp"

class EnvMock : public Env {
public:
    explicit EnvMock(double scaling_coeff = 0.) : calls_(0), coeff_((float)scaling_coeff) {}

    std::string get_action_space() override { return Env::SPACE_CONTINOUS; }
    std::string get_observation_space() override { return Env::SPACE_CONTINOUS; }
    int get_action_space_size() override { return kDim; }
    int get_observation_space_size() override { return kDim; }

    Mat reset() override { return filled(get_num_envs(), kDim); }

    std::vector<Mat> step(const Mat& /*actions*/) override {
        ++calls_;
        Mat dones = Mat::Zero(get_num_envs(), 1);
        if (calls_ % 300 == 0) dones = Mat::Ones(get_num_envs(), 1);
        return {filled(get_num_envs(), kDim), filled(get_num_envs(), 1), dones};
    }

    Mat get_original_obs() override { return filled(get_num_envs(), kDim); }
    Mat get_original_rew() override { return filled(get_num_envs(), 1); }
    void serialize(nlohmann::json&) override {}
    void deserialize(nlohmann::json&) override {}
    void render() override {}
    float get_time() override { return 0.f; }

private:
    static constexpr int kDim = 18;
    Mat filled(int r, int c) const { Mat m = Mat::Zero(r, c); for (long i = 0; i < (long)r * c; ++i) m.data()[i] = coeff_; return m; }
    long calls_;
    float coeff_;
};

namespace ppo_detail {
inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
inline uint64_t ctr_key(uint32_t seed, uint32_t env) { return splitmix64(((uint64_t)seed << 32) | env); }      // the (seed, env) half of the hash
inline uint32_t ctr_hash_keyed(uint64_t key, uint32_t step, uint32_t lane) { return (uint32_t)(splitmix64(key ^ (((uint64_t)step << 32) | lane)) >> 32); }
inline uint32_t ctr_hash(uint32_t seed, uint32_t env, uint32_t step, uint32_t lane) { return ctr_hash_keyed(ctr_key(seed, env), step, lane); }
inline float sym_unit(uint32_t h) { return (float)(h >> 8) * (1.0f / 8388608.0f) - 1.0f; }
}  // namespace ppo_detail

class SeededEnvMock : public Env {
public:
    // obs_dim / act_dim: 18 / 18 like EnvMock; 36 / 18 stands in for the hexapod that also observes its velocities
    // (reference env/hexapod_closed_loop_env.hpp:20).  Hash lanes 0 .. obs_dim-1 = the observation, obs_dim = reward, obs_dim + 1 = done.
    SeededEnvMock(uint32_t seed, uint32_t env_id, int obs_dim = 18, int act_dim = 18)
        : seed_(seed), id_(env_id), step_(0), last_rew_(0.f), key_(ppo_detail::ctr_key(seed, env_id)), kDim(obs_dim), kAct(act_dim) {}
    std::string get_action_space() override { return Env::SPACE_CONTINOUS; }
    std::string get_observation_space() override { return Env::SPACE_CONTINOUS; }
    int get_action_space_size() override { return kAct; }
    int get_observation_space_size() override { return kDim; }
    Mat reset() override { step_ = 0; return obs_at(0); }
    std::vector<Mat> step(const Mat& /*actions*/) override {
        ++step_;
        Mat rew(1, 1), done(1, 1);
        last_rew_ = ppo_detail::sym_unit(ppo_detail::ctr_hash_keyed(key_, step_, kDim));
        rew(0, 0) = last_rew_;
        done(0, 0) = (ppo_detail::ctr_hash_keyed(key_, step_, kDim + 1) % 300u == 0u) ? 1.f : 0.f;
        std::vector<Mat> out;             // (a braced list would COPY the three matrices into the vector: three more allocations per env step)
        out.reserve(3);
        out.push_back(obs_at(step_)); out.push_back(std::move(rew)); out.push_back(std::move(done));
        return out;
    }
    Mat get_original_obs() override { return obs_at(step_); }
    Mat get_original_rew() override { Mat r(1, 1); r(0, 0) = last_rew_; return r; }
    void serialize(nlohmann::json&) override {}
    void deserialize(nlohmann::json&) override {}
    void render() override {}
    float get_time() override { return 0.f; }

private:
    Mat obs_at(uint32_t step) const { Mat m(1, kDim); for (int j = 0; j < kDim; ++j) m(0, j) = ppo_detail::sym_unit(ppo_detail::ctr_hash_keyed(key_, step, (uint32_t)j)); return m; }
    uint32_t seed_, id_, step_;
    float last_rew_;
    uint64_t key_;                  // splitmix64(seed, env id): the step-independent half of the counter hash
    int kDim, kAct;
};

class TargetEnv : public Env {
public:
    TargetEnv(uint32_t seed, uint32_t env_id, int obs_dim = 18, int act_dim = 18, int episode_len = 100)
        : step_(0), last_rew_(0.f), key_(ppo_detail::ctr_key(seed, env_id)), kDim(obs_dim), kAct(act_dim), len_(episode_len), w_((size_t)act_dim * obs_dim) {
        const uint64_t wkey = ppo_detail::splitmix64(((uint64_t)seed << 32) | 0xffffffffull);       // one W per seed, shared by every environment of the job
        for (int j = 0; j < kAct; ++j)
            for (int k = 0; k < kDim; ++k) w_[(size_t)j * kDim + k] = 0.5f * ppo_detail::sym_unit((uint32_t)(ppo_detail::splitmix64(wkey ^ (((uint64_t)j << 32) | (uint32_t)k)) >> 32));
    }
    std::string get_action_space() override { return Env::SPACE_CONTINOUS; }
    std::string get_observation_space() override { return Env::SPACE_CONTINOUS; }
    int get_action_space_size() override { return kAct; }
    int get_observation_space_size() override { return kDim; }
    Mat reset() override { step_ = 0; return obs_at(0); }
    std::vector<Mat> step(const Mat& actions) override {
        const Mat cur = obs_at(step_);                       // the observation the action answers
        float acc = 0.f;
        for (int j = 0; j < kAct; ++j) {
            float tgt = 0.f;
            for (int k = 0; k < kDim; ++k) tgt += w_[(size_t)j * kDim + k] * cur(0, k);
            const float d = actions(0, j) - tgt;
            acc += d * d;
        }
        last_rew_ = -acc / (float)kAct;
        ++step_;
        Mat rew(1, 1), done(1, 1);
        rew(0, 0) = last_rew_;
        done(0, 0) = (step_ % (uint32_t)len_ == 0u) ? 1.f : 0.f;
        std::vector<Mat> out;
        out.reserve(3);
        out.push_back(obs_at(step_)); out.push_back(std::move(rew)); out.push_back(std::move(done));
        return out;
    }
    Mat get_original_obs() override { return obs_at(step_); }
    Mat get_original_rew() override { Mat r(1, 1); r(0, 0) = last_rew_; return r; }
    void serialize(nlohmann::json&) override {}
    void deserialize(nlohmann::json&) override {}
    void render() override {}
    float get_time() override { return 0.f; }

private:
    Mat obs_at(uint32_t step) const { Mat m(1, kDim); for (int j = 0; j < kDim; ++j) m(0, j) = ppo_detail::sym_unit(ppo_detail::ctr_hash_keyed(key_, step, (uint32_t)j)); return m; }
    uint32_t step_;
    float last_rew_;
    uint64_t key_;
    int kDim, kAct, len_;
    std::vector<float> w_;          // [act][obs], row-major
};

class DiscreteTargetEnv : public Env {
public:
    DiscreteTargetEnv(uint32_t seed, uint32_t env_id, int obs_dim = 18, int n_actions = 18, int episode_len = 100)
        : step_(0), last_rew_(0.f), key_(ppo_detail::ctr_key(seed, env_id)), kDim(obs_dim), kAct(n_actions), len_(episode_len), w_((size_t)n_actions * obs_dim) {
        const uint64_t wkey = ppo_detail::splitmix64(((uint64_t)seed << 32) | 0xffffffffull);       // TargetEnv's W
        for (int j = 0; j < kAct; ++j)
            for (int k = 0; k < kDim; ++k) w_[(size_t)j * kDim + k] = 0.5f * ppo_detail::sym_unit((uint32_t)(ppo_detail::splitmix64(wkey ^ (((uint64_t)j << 32) | (uint32_t)k)) >> 32));
    }
    std::string get_action_space() override { return Env::SPACE_DISCRETE; }
    std::string get_observation_space() override { return Env::SPACE_CONTINOUS; }
    int get_action_space_size() override { return kAct; }
    int get_observation_space_size() override { return kDim; }
    Mat reset() override { step_ = 0; return obs_at(0); }
    std::vector<Mat> step(const Mat& actions) override {
        const Mat cur = obs_at(step_);                       // the observation the action answers
        int best = 0; float best_v = 0.f;
        for (int j = 0; j < kAct; ++j) {
            float tgt = 0.f;
            for (int k = 0; k < kDim; ++k) tgt += w_[(size_t)j * kDim + k] * cur(0, k);
            if (j == 0 || tgt > best_v) { best = j; best_v = tgt; }
        }
        last_rew_ = (int)actions(0, 0) == best ? 1.f : 0.f;
        ++step_;
        Mat rew(1, 1), done(1, 1);
        rew(0, 0) = last_rew_;
        done(0, 0) = (step_ % (uint32_t)len_ == 0u) ? 1.f : 0.f;
        std::vector<Mat> out;
        out.reserve(3);
        out.push_back(obs_at(step_)); out.push_back(std::move(rew)); out.push_back(std::move(done));
        return out;
    }
    Mat get_original_obs() override { return obs_at(step_); }
    Mat get_original_rew() override { Mat r(1, 1); r(0, 0) = last_rew_; return r; }
    void serialize(nlohmann::json&) override {}
    void deserialize(nlohmann::json&) override {}
    void render() override {}
    float get_time() override { return 0.f; }

private:
    Mat obs_at(uint32_t step) const { Mat m(1, kDim); for (int j = 0; j < kDim; ++j) m(0, j) = ppo_detail::sym_unit(ppo_detail::ctr_hash_keyed(key_, step, (uint32_t)j)); return m; }
    uint32_t step_;
    float last_rew_;
    uint64_t key_;
    int kDim, kAct, len_;
    std::vector<float> w_;          // [category][obs], row-major
};

class MultiBinaryTargetEnv : public Env, public IMultiBinary {
public:
    MultiBinaryTargetEnv(uint32_t seed, uint32_t env_id, int obs_dim = 18, int n_bits = 18, int episode_len = 100)
        : step_(0), last_rew_(0.f), key_(ppo_detail::ctr_key(seed, env_id)), kDim(obs_dim), kAct(n_bits), len_(episode_len), w_((size_t)n_bits * obs_dim) {
        const uint64_t wkey = ppo_detail::splitmix64(((uint64_t)seed << 32) | 0xffffffffull);       // TargetEnv's W
        for (int j = 0; j < kAct; ++j)
            for (int k = 0; k < kDim; ++k) w_[(size_t)j * kDim + k] = 0.5f * ppo_detail::sym_unit((uint32_t)(ppo_detail::splitmix64(wkey ^ (((uint64_t)j << 32) | (uint32_t)k)) >> 32));
    }
    std::string get_action_space() override { return Env::SPACE_DISCRETE; }
    std::string get_observation_space() override { return Env::SPACE_CONTINOUS; }
    int get_action_space_size() override { return kAct; }
    int get_observation_space_size() override { return kDim; }
    Mat reset() override { step_ = 0; return obs_at(0); }
    std::vector<Mat> step(const Mat& actions) override {
        const Mat cur = obs_at(step_);                       // the observation the action answers
        int hits = 0;
        for (int j = 0; j < kAct; ++j) {
            float tgt = 0.f;
            for (int k = 0; k < kDim; ++k) tgt += w_[(size_t)j * kDim + k] * cur(0, k);
            if ((actions(0, j) != 0.f) == (tgt > 0.f)) ++hits;
        }
        last_rew_ = (float)hits / (float)kAct;
        ++step_;
        Mat rew(1, 1), done(1, 1);
        rew(0, 0) = last_rew_;
        done(0, 0) = (step_ % (uint32_t)len_ == 0u) ? 1.f : 0.f;
        std::vector<Mat> out;
        out.reserve(3);
        out.push_back(obs_at(step_)); out.push_back(std::move(rew)); out.push_back(std::move(done));
        return out;
    }
    Mat get_original_obs() override { return obs_at(step_); }
    Mat get_original_rew() override { Mat r(1, 1); r(0, 0) = last_rew_; return r; }
    void serialize(nlohmann::json&) override {}
    void deserialize(nlohmann::json&) override {}
    void render() override {}
    float get_time() override { return 0.f; }

private:
    Mat obs_at(uint32_t step) const { Mat m(1, kDim); for (int j = 0; j < kDim; ++j) m(0, j) = ppo_detail::sym_unit(ppo_detail::ctr_hash_keyed(key_, step, (uint32_t)j)); return m; }
    uint32_t step_;
    float last_rew_;
    uint64_t key_;
    int kDim, kAct, len_;
    std::vector<float> w_;          // [bit][obs], row-major
};

class MaskedTargetEnv : public Env, public IActionMask {
public:
    MaskedTargetEnv(uint32_t seed, uint32_t env_id, int obs_dim = 18, int n_actions = 18, int episode_len = 100)
        : step_(0), last_rew_(0.f), forbidden_(0), key_(ppo_detail::ctr_key(seed, env_id)), kDim(obs_dim), kAct(n_actions), len_(episode_len), w_((size_t)n_actions * obs_dim) {
        const uint64_t wkey = ppo_detail::splitmix64(((uint64_t)seed << 32) | 0xffffffffull);       // TargetEnv's W
        for (int j = 0; j < kAct; ++j)
            for (int k = 0; k < kDim; ++k) w_[(size_t)j * kDim + k] = 0.5f * ppo_detail::sym_unit((uint32_t)(ppo_detail::splitmix64(wkey ^ (((uint64_t)j << 32) | (uint32_t)k)) >> 32));
    }
    std::string get_action_space() override { return Env::SPACE_DISCRETE; }
    std::string get_observation_space() override { return Env::SPACE_CONTINOUS; }
    int get_action_space_size() override { return kAct; }
    int get_observation_space_size() override { return kDim; }
    Mat reset() override { step_ = 0; return obs_at(0); }
    std::vector<Mat> step(const Mat& actions) override {
        const int a = (int)actions(0, 0), best = target_at(step_);     // for the observation the action answers
        const bool legal = a >= 0 && a < kAct && allowed_at(step_, a, best);
        if (!legal) ++forbidden_;
        last_rew_ = !legal ? -1.f : a == best ? 1.f : 0.f;
        ++step_;
        Mat rew(1, 1), done(1, 1);
        rew(0, 0) = last_rew_;
        done(0, 0) = (step_ % (uint32_t)len_ == 0u) ? 1.f : 0.f;
        std::vector<Mat> out;
        out.reserve(3);
        out.push_back(obs_at(step_)); out.push_back(std::move(rew)); out.push_back(std::move(done));
        return out;
    }
    // legality of the categories for the current observation obs_at(step_)
    Mat get_action_mask() override {
        Mat m(1, kAct);
        const int best = target_at(step_);
        for (int j = 0; j < kAct; ++j) m(0, j) = allowed_at(step_, j, best) ? 1.f : 0.f;
        return m;
    }
    long forbidden_received() const { return forbidden_; }
    int target() const { return target_at(step_); }
    Mat get_original_obs() override { return obs_at(step_); }
    Mat get_original_rew() override { Mat r(1, 1); r(0, 0) = last_rew_; return r; }
    void serialize(nlohmann::json&) override {}
    void deserialize(nlohmann::json&) override {}
    void render() override {}
    float get_time() override { return 0.f; }

private:
    Mat obs_at(uint32_t step) const { Mat m(1, kDim); for (int j = 0; j < kDim; ++j) m(0, j) = ppo_detail::sym_unit(ppo_detail::ctr_hash_keyed(key_, step, (uint32_t)j)); return m; }
    int target_at(uint32_t step) const {
        const Mat cur = obs_at(step);
        int best = 0; float best_v = 0.f;
        for (int j = 0; j < kAct; ++j) {
            float tgt = 0.f;
            for (int k = 0; k < kDim; ++k) tgt += w_[(size_t)j * kDim + k] * cur(0, k);
            if (j == 0 || tgt > best_v) { best = j; best_v = tgt; }
        }
        return best;
    }
    // the top bit of the stream's word (step, obs_dim + j) forbids category j; the target is always allowed
    bool allowed_at(uint32_t step, int j, int best) const { return j == best || (ppo_detail::ctr_hash_keyed(key_, step, (uint32_t)(kDim + j)) >> 31) == 0u; }
    uint32_t step_;
    float last_rew_;
    long forbidden_;
    uint64_t key_;
    int kDim, kAct, len_;
    std::vector<float> w_;          // [category][obs], row-major
};

class MultiDiscreteTargetEnv : public Env, public IMultiDiscrete, public IActionMask {
public:
    MultiDiscreteTargetEnv(uint32_t seed, uint32_t env_id, int obs_dim, const std::vector<int>& nvec, int episode_len = 100, bool masked = false)
        : step_(0), last_rew_(0.f), forbidden_(0), key_(ppo_detail::ctr_key(seed, env_id)), kDim(obs_dim), len_(episode_len), masked_(masked), nvec_(nvec), off_(nvec.size() + 1, 0) {
        for (size_t k = 0; k < nvec_.size(); ++k) off_[k + 1] = off_[k] + nvec_[k];
        w_.resize((size_t)off_.back() * kDim);
        const uint64_t wkey = ppo_detail::splitmix64(((uint64_t)seed << 32) | 0xffffffffull);       // TargetEnv's key; component k hashes under wkey ^ ((k + 1) << 48)
        for (size_t k = 0; k < nvec_.size(); ++k) {
            const uint64_t ck = ppo_detail::splitmix64(wkey ^ ((uint64_t)(k + 1) << 48));
            for (int j = 0; j < nvec_[k]; ++j)
                for (int i = 0; i < kDim; ++i)
                    w_[(size_t)(off_[k] + j) * kDim + i] = 0.5f * ppo_detail::sym_unit((uint32_t)(ppo_detail::splitmix64(ck ^ (((uint64_t)j << 32) | (uint32_t)i)) >> 32));
        }
    }
    std::string get_action_space() override { return Env::SPACE_DISCRETE; }
    std::string get_observation_space() override { return Env::SPACE_CONTINOUS; }
    int get_action_space_size() override { return off_.back(); }           // A = sum of the components' widths
    int get_observation_space_size() override { return kDim; }
    std::vector<int> get_action_nvec() override { return nvec_; }
    Mat reset() override { step_ = 0; return obs_at(0); }
    std::vector<Mat> step(const Mat& actions) override {
        const int K = (int)nvec_.size();
        const std::vector<int> best = targets_at(step_);      // for the observation the action answers
        int hits = 0; bool legal = true;
        for (int k = 0; k < K; ++k) {
            const int a = (int)actions(0, k);
            if (a == best[k]) ++hits;
            if (masked_ && !(a >= 0 && a < nvec_[k] && allowed_at(step_, off_[k] + a, off_[k] + best[k]))) legal = false;
        }
        if (!legal) ++forbidden_;
        last_rew_ = legal ? (float)hits / (float)K : -1.f;
        ++step_;
        Mat rew(1, 1), done(1, 1);
        rew(0, 0) = last_rew_;
        done(0, 0) = (step_ % (uint32_t)len_ == 0u) ? 1.f : 0.f;
        std::vector<Mat> out;
        out.reserve(3);
        out.push_back(obs_at(step_)); out.push_back(std::move(rew)); out.push_back(std::move(done));
        return out;
    }
    // legality of every column for the current observation obs_at(step_): [1, A]
    Mat get_action_mask() override {
        Mat m = Mat::Ones(1, off_.back());
        if (!masked_) return m;
        const std::vector<int> best = targets_at(step_);
        for (size_t k = 0; k < nvec_.size(); ++k)
            for (int j = off_[k]; j < off_[k + 1]; ++j) m(0, j) = allowed_at(step_, j, off_[k] + best[k]) ? 1.f : 0.f;
        return m;
    }
    bool has_action_mask() override { return masked_; }
    long forbidden_received() const { return forbidden_; }
    std::vector<int> targets() const { return targets_at(step_); }
    Mat get_original_obs() override { return obs_at(step_); }
    Mat get_original_rew() override { Mat r(1, 1); r(0, 0) = last_rew_; return r; }
    void serialize(nlohmann::json&) override {}
    void deserialize(nlohmann::json&) override {}
    void render() override {}
    float get_time() override { return 0.f; }

private:
    Mat obs_at(uint32_t step) const { Mat m(1, kDim); for (int j = 0; j < kDim; ++j) m(0, j) = ppo_detail::sym_unit(ppo_detail::ctr_hash_keyed(key_, step, (uint32_t)j)); return m; }
    std::vector<int> targets_at(uint32_t step) const {
        const Mat cur = obs_at(step);
        std::vector<int> best(nvec_.size(), 0);
        for (size_t k = 0; k < nvec_.size(); ++k) {
            float best_v = 0.f;
            for (int j = 0; j < nvec_[k]; ++j) {
                float tgt = 0.f;
                for (int i = 0; i < kDim; ++i) tgt += w_[(size_t)(off_[k] + j) * kDim + i] * cur(0, i);
                if (j == 0 || tgt > best_v) { best[k] = j; best_v = tgt; }
            }
        }
        return best;
    }
    // the top bit of the stream's word (step, obs_dim + column) forbids the column; a component's target is always allowed
    bool allowed_at(uint32_t step, int col, int best_col) const { return col == best_col || (ppo_detail::ctr_hash_keyed(key_, step, (uint32_t)(kDim + col)) >> 31) == 0u; }
    uint32_t step_;
    float last_rew_;
    long forbidden_;
    uint64_t key_;
    int kDim, len_;
    bool masked_;
    std::vector<int> nvec_, off_;
    std::vector<float> w_;          // [column][obs], row-major; component k's rows start at off_[k]
};

class UnitRewardEnv : public Env {
public:
    UnitRewardEnv(uint32_t seed, uint32_t env_id, int obs_dim = 18, int act_dim = 18) : step_(0), key_(ppo_detail::ctr_key(seed, env_id)), kDim(obs_dim), kAct(act_dim) {}
    std::string get_action_space() override { return Env::SPACE_CONTINOUS; }
    std::string get_observation_space() override { return Env::SPACE_CONTINOUS; }
    int get_action_space_size() override { return kAct; }
    int get_observation_space_size() override { return kDim; }
    Mat reset() override { ++step_; return obs_at(step_); }
    std::vector<Mat> step(const Mat& /*actions*/) override {
        ++step_;
        std::vector<Mat> out;
        out.reserve(3);
        out.push_back(obs_at(step_)); out.push_back(Mat::Ones(1, 1)); out.push_back(Mat::Zero(1, 1));
        return out;
    }
    Mat get_original_obs() override { return obs_at(step_); }
    Mat get_original_rew() override { return Mat::Ones(1, 1); }
    void serialize(nlohmann::json&) override {}
    void deserialize(nlohmann::json&) override {}
    void render() override {}
    float get_time() override { return 0.f; }

private:
    Mat obs_at(uint32_t step) const { Mat m(1, kDim); for (int j = 0; j < kDim; ++j) m(0, j) = ppo_detail::sym_unit(ppo_detail::ctr_hash_keyed(key_, step, (uint32_t)j)); return m; }
    uint32_t step_;
    uint64_t key_;
    int kDim, kAct;
};
