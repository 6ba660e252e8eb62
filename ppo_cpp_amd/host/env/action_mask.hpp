// action_mask.hpp -- state-dependent legality of discrete actions as an OPTIONAL mixin beside the Env interface, in the style of time_limit.hpp (no reference
// counterpart: the reference's environments are continuous-control; sb3-contrib's MaskablePPO is the usual statement of invalid-action masking).
//
// Env itself stays the reference's interface.  A SPACE_DISCRETE environment (or wrapper) that ALSO derives from IActionMask tells the algorithm which categories are
// legal for its CURRENT observation.  PPO2 / Runner look for the mixin with dynamic_cast, turn masking on for the handle (ppo_set_action_masking) and then sample, train
// and play back under the masks (ppo_rollout_act_masked / ppo_step_masked / ppo_train_step_masked / ppo_act_deterministic_masked in include/ppo_hip.h); an Env
// without it behaves as before.
//   VecEnv and EnvNormalize forward the mixin from their children (vec_env.hpp, env_normalize.hpp); children without it report all categories allowed.
#pragma once
#include "env.hpp"

struct IActionMask {
    virtual ~IActionMask() {}
    // [n_envs, A]: non-zero = category allowed for the current observation (the one reset() or the last step() returned); every row allows at least one category.
    // Valid after reset() and after every step().
    virtual Mat get_action_mask() = 0;
    // a container (VecEnv, EnvNormalize) always carries the mixin: false when nothing inside it masks, so that callers keep the unmasked path
    virtual bool has_action_mask() { return true; }
};
