// multi_discrete.hpp -- a multi-discrete action space (several independent choices per step) as an OPTIONAL mixin beside the Env interface, in the style of
// action_mask.hpp / time_limit.hpp (no reference counterpart: the reference's environments are continuous-control; stable-baselines states the matching
// distribution as MultiCategoricalProbabilityDistribution).
//
// Env itself stays the reference's interface.  A SPACE_DISCRETE environment (or wrapper) that ALSO derives from IMultiDiscrete has K components of n_0 .. n_{K-1}
// categories: its get_action_space_size() is A = n_0 + .. + n_{K-1} (noise and mask matrices keep their [n_envs, A] shape, component k owning columns
// [o_k, o_k + n_k)), and it takes actions [n_envs, K], column k = the index WITHIN component k.  PPO2 looks for the mixin with dynamic_cast and serves such an Env with
// a multi-categorical handle (ppo_create_multi in include/ppo_hip.h; PPO2::create_handle picks it); an Env without it behaves as before.
//   VecEnv, EnvNormalize and TimeLimit forward the mixin from their children (vec_env.hpp, env_normalize.hpp, time_limit.hpp); a VecEnv whose children disagree
//   about their components is refused.
#pragma once
#include <vector>

#include "env.hpp"

struct IMultiDiscrete {
    virtual ~IMultiDiscrete() {}
    // categories per component, in column order
    virtual std::vector<int> get_action_nvec() = 0;
    // a container (VecEnv, EnvNormalize, TimeLimit) always carries the mixin: false when nothing inside it is multi-discrete
    virtual bool has_action_nvec() { return true; }
};

// the components of `env`, or an empty vector when it is not multi-discrete
inline std::vector<int> action_nvec_of(Env* env) {
    IMultiDiscrete* md = dynamic_cast<IMultiDiscrete*>(env);
    return md && md->has_action_nvec() ? md->get_action_nvec() : std::vector<int>();
}
