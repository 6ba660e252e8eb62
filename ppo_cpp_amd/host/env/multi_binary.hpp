// multi_binary.hpp -- a multi-binary action space (A independent on / off decisions per step) as an OPTIONAL mixin beside the Env interface, in the style of
// multi_discrete.hpp / action_mask.hpp / time_limit.hpp (no reference counterpart: the reference's environments are continuous-control; stable-baselines states the
// matching distribution as BernoulliProbabilityDistribution over a MultiBinary space).
//
// Env itself stays the reference's interface.  A SPACE_DISCRETE environment (or wrapper) that ALSO derives from IMultiBinary has A bits: its
// get_action_space_size() is A, and it takes actions [n_envs, A], every element exactly 0 or 1.  PPO2 looks for the mixin with dynamic_cast and serves such an Env
// with a multi-binary handle (PPO_ACT_MULTI_BINARY in include/ppo_hip.h; PPO2::action_dist_for / create_handle pick it); an Env without it behaves as before.
//   VecEnv, EnvNormalize and TimeLimit forward the mixin from their children (vec_env.hpp, env_normalize.hpp, time_limit.hpp); a VecEnv whose children disagree
//   is refused, and so is an Env that is both multi-discrete (multi_discrete.hpp) and multi-binary.  Action masks (action_mask.hpp) do not apply to this space.
#pragma once
#include "env.hpp"

struct IMultiBinary {
    virtual ~IMultiBinary() {}
    // a container (VecEnv, EnvNormalize, TimeLimit) always carries the mixin: false when nothing inside it is multi-binary
    virtual bool has_binary_actions() { return true; }
};

// whether `env` takes multi-binary actions
inline bool binary_actions_of(Env* env) {
    IMultiBinary* mb = dynamic_cast<IMultiBinary*>(env);
    return mb && mb->has_binary_actions();
}
