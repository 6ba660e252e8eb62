// ppo_envnorm.hpp -- the ONE home of EnvNormalize::step's and RunningStatistics::update's per-column / per-element arithmetic and of the seeded env's transition.
// The rollout kernels (narrow_collect / rollout / host_step / rollout_coop, rollout1, norm_batch, obs_normalize, seeded_env) keep their own lanes, loops over
// environments, barriers, LDS blocks and stores and call these pieces for the formulas: plain floats, doubles and ints in and out, no lane index, no barrier, no
// argument struct.  `file:line` citations are the reference's.  Operand order and association are the reference's; the build does not contract
// (-ffp-contract=off), so a call site gets the bits of the expression written out in place.
// As with ppo_head.hpp a call must also leave its kernel's MACHINE CODE alone (tools/kernel_code_diff.py).  The compiler simplifies a piece before it inlines it:
// hence no piece with a loop (the two passes of the batch moments, the return recurrence and the reward row stay loops of their kernels: as pieces they came
// out with other registers and more spills in the persistent kernels), and two forms of the observation scale around where 1 / sqrt(var + eps) is evaluated.
// Included by ppo_kernels.hpp (after tf_min / tf_max and the counter hash), which every other header sees.
#pragma once

// ---- RunningStatistics::update (common/running_statistics.hpp:51-54, 88-104) ---------------------------------------------------------------------------------
// The merge of a batch (bmean, bM2 = its sum of squared deviations, nb rows) into (mean0, var0, cnt rows).  The caller bumps the count: cnt = (double)nb + cnt (:103).
__device__ __forceinline__ void rs_merge(float mean0, float var0, double cnt, float bmean, float bM2, float nbf, float& mean1, float& var1) {
    const double nb = (double)nbf, tot = cnt + nb;
    const float bvar = bM2 / (float)nb;                                        // :51-54
    const float delta = bmean - mean0;                                         // :90
    mean1 = mean0 + (delta * (float)nb) / (float)tot;                          // :94
    const float m_a = var0 * (float)cnt, m_b = bvar * (float)nb;               // :97-98
    const float M2 = m_a + m_b + (((delta * delta) * (float)cnt) * (float)nb) / (float)tot;   // :100
    var1 = M2 / (float)tot;                                                    // :101
}

// ---- EnvNormalize (env/env_normalize.hpp:64-116) ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float en_istd(float var, float eps) { return 1.0f / sqrtf(var + eps); }                        // :79, :101
// An observation, normalised and clipped (:99-104), in two forms.  obs_scale: with istd = en_istd(var, eps) kept per column by the resident kernels, which evaluate
// it once per statistics update; obs_scale_var: from the variance, for the per-step kernels.  Both evaluate the same expression, hence the same rounding.
__device__ __forceinline__ float obs_scale(float x, float mean, float istd, float clip) {
    x = (x - mean) * istd;
    return tf_min(tf_max(x, -clip), clip);
}
__device__ __forceinline__ float obs_scale_var(float x, float mean, float var, float eps, float clip) {
    x = (x - mean) * en_istd(var, eps);
    return tf_min(tf_max(x, -clip), clip);
}
// A reward, scaled with inv = en_istd of the returns' variance and clipped (:75-87; as it is when the reward branch is off), and a return behind its done flag (:88-91).
// The return recurrence in front of them is ret = ret * gamma + r (:66), a loop of its kernel.
__device__ __forceinline__ float en_reward(float r, float inv, int norm_rew, float clip) {
    float y = r;
    if (norm_rew) { y = y * inv; y = tf_min(tf_max(y, -clip), clip); }
    return y;
}
__device__ __forceinline__ float en_ret_reset(float ret, float done) { return ret * (1.0f - done); }

// ---- the seeded synthetic env (oracle/ppo_oracle.c orc_seeded_env_step; stands in for env/env_mock.hpp) --------------------------------------------------------
// Environment `env` at env step `step` has O + 2 hash words: j < O the observation, j == O the reward, j == O + 1 the done flag (one step in 300).
__device__ __forceinline__ uint32_t seeded_env_word(uint32_t seed, int env, uint32_t step, int j) { return ctr_hash(seed, (uint32_t)env, step, (uint32_t)j); }
// element i of a block of environments [env0, ..) x (O + 2) words -> its environment e (from env0), its j and its word
__device__ __forceinline__ uint32_t seeded_env_elem(uint32_t seed, int env0, uint32_t step, int i, int O, int& e, int& j) {
    e = i / (O + 2); j = i - e * (O + 2);
    return seeded_env_word(seed, env0 + e, step, j);
}
__device__ __forceinline__ float seeded_value(uint32_t h) { return u32_to_sym_unit(h); }                                  // an observation or the reward
__device__ __forceinline__ float seeded_done(uint32_t h) { return (h % 300u == 0u) ? 1.0f : 0.0f; }
