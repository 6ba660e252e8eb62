// ppo_head.hpp -- the ONE home of the policy head's and the surrogate loss's per-row / per-element arithmetic.  Every kernel family (policy_step / train_fwd_bwd, the narrow kernels, rollout1, train8, the bf16 sample / loss kernels) keeps its own lanes, loops, register
// arrays, reductions, loads and stores and calls these pieces for the formulas: plain floats, ints and bools in and out, no lane index, no LDS, no argument
// struct.  A reference-graph citation ("G:", see ppo_kernels.hpp) and a tie or NaN rule is written here.  Operand order and association are the graph's; the
// build does not contract (-ffp-contract=off), so a call site gets the bits of the expression written out in place.
// A call must also leave its kernel's MACHINE CODE alone (tools/kernel_code_diff.py): a piece is simplified before it is inlined, so it keeps the statement order
// of the code it replaces -- hence two surrogate pieces around the caller's read of 1/n, loss terms stored by their piece, a few marked sites left written out.
// Included by ppo_kernels.hpp (after tf_min / tf_max), which every other header sees.
#pragma once

#define HALF_LOG_2PI 0.9189385175704956f   /* G:6531 */
#define HALF_LOG_2PIE 1.4189385175704956f  /* G:10021-10180 */

// ---- clipped surrogate of one row (G:9428-11290) and d loss / d neglogp (G:12609-22656) ---------------------------------------------------------------------
// A dead row of the last tile (live == false) comes with adv = 0 and old_nlp = nlp and contributes zeros.
struct SurrogateRow { float lo, hi, ratio, rmin, m1, m2; };           // the loss is max(m1, m2)
__device__ __forceinline__ SurrogateRow surrogate_row(float nlp, float old_nlp, float adv, float cr) {
    const float lo = 1.0f - cr, hi = 1.0f + cr;
    const float ratio = expf(old_nlp - nlp);
    const float rmin = tf_min(ratio, hi);
    const float rclip = tf_max(rmin, lo);
    return {lo, hi, ratio, rmin, -adv * ratio, -adv * rclip};
}
// g = 1 / (minibatch rows), the gradient of the Mean nodes
__device__ __forceinline__ float surrogate_d_nlp(SurrogateRow s, float adv, float g, bool live) {
    const float sel = (s.m1 >= s.m2) ? 1.0f : 0.0f;                                          // Maximum tie rule G:12609
    const float pass = ((s.rmin >= s.lo) ? 1.0f : 0.0f) * ((s.ratio <= s.hi) ? 1.0f : 0.0f); // G:15357, 16113
    float d_ratio = (-adv) * g * sel;
    d_ratio += (-adv) * g * (1.0f - sel) * pass;
    return live ? -(d_ratio * s.ratio) : 0.0f;
}
// Row r's loss terms {policy loss, entropy, (nlp - old_nlp)^2, clipped?} -> t[4 r .. 4 r + 3], called by the ONE lane of the row that stores them
__device__ __forceinline__ void surrogate_terms(SurrogateRow s, float nlp, float old_nlp, float ent, float cr, bool live, float* t, int r) {
    const float dk = nlp - old_nlp;
    t[r * 4 + 0] = live ? tf_max(s.m1, s.m2) : 0.f;
    t[r * 4 + 1] = live ? ent : 0.f;
    t[r * 4 + 2] = live ? dk * dk : 0.f;
    t[r * 4 + 3] = (live && fabsf(s.ratio - 1.0f) > cr) ? 1.0f : 0.f;
}

// ---- diagonal Gaussian head (G:5894-6672 act model, G:9428-10180 train model) --------------------------------------------------------------------------------
// One element: logstd is the graph's `mu * 0 + logstd` broadcast (a NaN or infinite mu reaches logstd, as in the graph), sigma = exp(logstd); the act model draws
// act = mu + sigma eps; z = (act - mu) / sigma.
__device__ __forceinline__ float gauss_logstd(float mu, float ls) { return mu * 0.0f + ls; }
struct GaussStd { float logstd, sigma; };
__device__ __forceinline__ GaussStd gauss_std(float mu, float ls) {
    const float logstd = gauss_logstd(mu, ls);
    return {logstd, expf(logstd)};
}
__device__ __forceinline__ float gauss_sample(float mu, float sigma, float eps) { return mu + sigma * eps; }
__device__ __forceinline__ float gauss_z(float act, float mu, float sigma) { return (act - mu) / sigma; }
// neglogp of a row from the reduced sums ssq = sum z^2, slog = sum logstd; an element's share of the entropy
__device__ __forceinline__ float gauss_nlp(float ssq, float slog, int A) { return 0.5f * ssq + HALF_LOG_2PI * (float)A + slog; }
__device__ __forceinline__ float gauss_entropy_elem(float logstd) { return logstd + HALF_LOG_2PIE; }
// d loss / d mu and d loss / d logstd of one element
__device__ __forceinline__ void gauss_grad_elem(float d_nlp, float z, float sigma, float ent_coef, float g, float& dmu, float& dl) {
    dl = d_nlp * (1.0f - z * z) - ent_coef * g;                                        // AddN_2 G:21299
    dmu = d_nlp * (-(z / sigma)) + dl * 0.0f;                                          // AddN_3 G:22656
}

// ---- categorical head (stable-baselines CategoricalProbabilityDistribution; per component for the multi-categorical one) -----------------------------------------
// a = argmax_j (l_j - log(-log u_j)); m = max_j l_j, a0 = l - m, z = sum_j exp(a0_j), neglogp = log z - a0[a], entropy = sum_j p_j (log z - a0_j): allowed j only
__device__ __forceinline__ float gumbel(float l, float u) { return l - logf(-logf(u)); }
// One candidate (v, j) -- a category that exists and is allowed: the caller asks -- against a lane's running (best, at) pair: a larger value wins, an equal one
// does not (the lower index stays: tf.argmax).  FIRST: the pair started at `none` ("none yet" = one past the end), so the first allowed category is taken even when
// its value is -inf (u == 0) and a lane without one loses every tie of the butterfly to a real index; the caller clamps a row without any (which the host checks
// refuse) afterwards.
template <bool FIRST>
__device__ __forceinline__ void cat_take(float v, int j, int none, float& best, int& at) {
    if (v > best || (FIRST && at == none)) { best = v; at = j; }
}
// category j's share of the entropy and d loss / d l_j = d_nlp (p_j - [j == a]) + ent_coef g p_j (log p_j + H), with ex = exp(a0), lz = log z, H the entropy of j's
// own component.  Forbidden and padding columns and dead rows are not passed here: the caller writes exactly +0 for them.
__device__ __forceinline__ float cat_entropy_term(float ex, float z, float lz, float a0) { return (ex / z) * (lz - a0); }
__device__ __forceinline__ float cat_grad_elem(float d_nlp, float ex, float z, float a0, float lz, float H, int j, int act, float ent_coef, float g) {
    const float p = ex / z;
    return d_nlp * (p - (j == act ? 1.0f : 0.0f)) + ent_coef * g * (p * ((a0 - lz) + H));
}

// ---- multi-binary head (stable-baselines BernoulliProbabilityDistribution: A independent on / off decisions over the logits l in place of mu) -----------------------
// One element, from e = exp(-|l|) (never overflows), sp = log1p(e) = softplus(-|l|), q = e / (1 + e) = the probability of the LESS likely value:
//   p = sigmoid(l) = l >= 0 ? 1 / (1 + e) : q;  sample x = u < p (u uniform in [0, 1): p == 1 always gives 1, p == 0 always 0);  deterministic x = l > 0, which is
//   tf.round(sigmoid(l)) -- a logit of +-0 gives 0
//   neglogp = sp + (x == (l > 0) ? 0 : |l|)      = TF's sigmoid_cross_entropy_with_logits(l, x) = relu(l) - l x + log1p(exp(-|l|))
//   entropy = sp + |l| q                         = the same expression with the label p
//   d loss / d l = d_nlp (p - x) + ent_coef g l p (1 - p), p (1 - p) = e / (1 + e)^2: the derivative of the SMOOTH identity softplus(l) - l x.  At a logit of exactly
//   +-0 TensorFlow's composed graph differentiates the relu and abs kinks to 0 and gives another value; this is the smooth one everywhere.
// Padding columns and dead rows are not passed here: the caller writes exactly +0 for them.
struct BernParts { float e, sp, q, p; };
__device__ __forceinline__ BernParts bern_parts(float l) {
    const float e = expf(-fabsf(l));
    const float q = e / (1.0f + e);
    return {e, log1pf(e), q, l >= 0.0f ? 1.0f / (1.0f + e) : q};
}
__device__ __forceinline__ float bern_sample(float p, float u) { return u < p ? 1.0f : 0.0f; }
__device__ __forceinline__ float bern_mode(float l) { return l > 0.0f ? 1.0f : 0.0f; }
__device__ __forceinline__ float bern_nlp_elem(BernParts b, float l, float x) { return b.sp + (((x != 0.0f) == (l > 0.0f)) ? 0.0f : fabsf(l)); }
__device__ __forceinline__ float bern_entropy_elem(BernParts b, float l) { return b.sp + fabsf(l) * b.q; }
__device__ __forceinline__ float bern_grad_elem(float d_nlp, BernParts b, float l, float x, float ent_coef, float g) {
    const float d = 1.0f + b.e;
    return d_nlp * (b.p - x) + ent_coef * g * (l * (b.e / (d * d)));
}
