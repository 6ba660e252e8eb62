// time_limit.hpp -- time-limit truncation as an OPTIONAL mixin beside the Env interface (no reference counterpart: the reference's
// environments end an episode because the clock ran out -- hexapod_closed_loop_env.hpp `done = get_time() >= simulation_duration` -- and its
// Runner::set_returns treats that like a terminal state).
//
// Env itself stays the reference's interface, so an existing environment keeps compiling.  An environment (or wrapper) that ALSO derives from
// ITimeLimit tells the algorithm which of the dones of its last step() were truncations, and hands over the observation those episodes ended
// on -- step() returns the observation AFTER the reset, as the Env contract says.  PPO2 / Runner look for the mixin with dynamic_cast and then
// bootstrap the value at those steps (ppo_rollout_mark_truncated / ppo_gae_ex in include/ppo_hip.h); an Env without it behaves as before.
//   TimeLimit   wraps any ONE-environment Env with max_episode_steps.
//   VecEnv and EnvNormalize forward the mixin from their children (vec_env.hpp, env_normalize.hpp).
//   TimeLimit forwards the multi-discrete mixin of the environment it wraps (multi_discrete.hpp), and the multi-binary one (multi_binary.hpp).
#pragma once
#include <memory>
#include <stdexcept>

#include "env.hpp"
#include "multi_binary.hpp"
#include "multi_discrete.hpp"

struct ITimeLimit {
    virtual ~ITimeLimit() {}
    // [n_envs, 1] of the last step(): 1 where the done was raised by the time limit, 0 where the episode terminated or goes on
    virtual Mat get_truncated() = 0;
    // [n_envs, obs] RAW observations the truncated episodes ended on; rows are valid where get_truncated() is 1
    virtual Mat get_terminal_obs() = 0;
    // a container (VecEnv, EnvNormalize) always carries the mixin: false when nothing inside it has a time limit, so that callers skip the per-step queries
    virtual bool has_time_limit() { return true; }
};

class TimeLimit : public Env, public ITimeLimit, public IMultiDiscrete, public IMultiBinary {
public:
    TimeLimit(std::shared_ptr<Env> env, int max_episode_steps)
        : env_(std::move(env)), limit_(max_episode_steps), steps_(0), truncated_(Mat::Zero(1, 1)), terminal_obs_(Mat::Zero(1, env_->get_observation_space_size())) {
        if (env_->get_num_envs() != 1) throw std::runtime_error("TimeLimit wraps one environment (put it inside the VecEnv)");
        if (limit_ < 1) throw std::runtime_error("TimeLimit: max_episode_steps must be positive");
    }

    std::string get_action_space() override { return env_->get_action_space(); }
    std::string get_observation_space() override { return env_->get_observation_space(); }
    int get_action_space_size() override { return env_->get_action_space_size(); }
    int get_observation_space_size() override { return env_->get_observation_space_size(); }

    Mat reset() override { steps_ = 0; truncated_(0, 0) = 0.f; return env_->reset(); }

    std::vector<Mat> step(const Mat& actions) override {
        std::vector<Mat> r = env_->step(actions);
        ++steps_;
        truncated_(0, 0) = 0.f;
        if (r[2](0, 0) != 0.f) { steps_ = 0; return r; }            // the inner env ended the episode by itself: a termination (it has reset itself, as the Env contract says)
        if (steps_ >= limit_) {
            terminal_obs_ = r[0];                                   // the observation the episode ends on
            truncated_(0, 0) = 1.f;
            r[0] = env_->reset();                                   // Env contract: the observation after the reset
            r[2](0, 0) = 1.f;
            steps_ = 0;
        }
        return r;
    }

    Mat get_truncated() override { return truncated_; }
    Mat get_terminal_obs() override { return terminal_obs_; }
    std::vector<int> get_action_nvec() override { return action_nvec_of(env_.get()); }
    bool has_action_nvec() override { return !action_nvec_of(env_.get()).empty(); }
    bool has_binary_actions() override { return binary_actions_of(env_.get()); }

    void render() override { env_->render(); }
    float get_time() override { return env_->get_time(); }
    Mat get_original_obs() override { return env_->get_original_obs(); }
    Mat get_original_rew() override { return env_->get_original_rew(); }
    void serialize(nlohmann::json& j) override { env_->serialize(j); }
    void deserialize(nlohmann::json& j) override { env_->deserialize(j); }
    Env& inner() { return *env_; }

private:
    std::shared_ptr<Env> env_;
    int limit_, steps_;
    Mat truncated_, terminal_obs_;
};
