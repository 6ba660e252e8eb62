/*
 * ppo_hip.h  --  C-ABI of libppo_hip.so: the MI355X (gfx950) replacement for the TensorFlow graph
 * executor behind ppo_cpp's rollout-collect + minibatch-update hot path.
 *
 * The reference has no plugin/FFI layer for this path: the seam is tensorflow::Session::Run addressed by
 * tensor-name strings (reference ppo2/ppo2.hpp:521-544).  Every entry point below replaces one of those
 * call sites (cited per function, paths relative to the reference root).  Plain pointers and sizes only;
 * no torch / Eigen / TF types.
 *
 * Conventions
 *   - all matrices are row-major fp32 (reference env/env.hpp:14 `Mat`), all vectors contiguous fp32
 *   - every pointer argument is HOST memory unless the name ends in _dev; the caller owns it and it is
 *     only used for the duration of the call (the reference copies on every call too: ppo2/utils.hpp:42,53)
 *   - return value: 0 = ok, negative = error; ppo_last_error() gives the message.  The reference prints
 *     status.ToString() and assert(false)s (ppo2/policies.hpp:39-43, ppo2/ppo2.hpp:452-456)
 *   - one handle = one caller thread = one HIP device + stream (reference: every Session::Run is issued
 *     from the single main thread, env worker threads never touch the session: env/vec_env.hpp:247)
 *   - a non-finite gradient norm poisons the weights with NaN exactly like G:24493-24543; not an error
 *   - there is NO CPU fallback: every call fails loudly when no gfx950 device is usable
 *   - PPO_F32 arithmetic: exact-fp32 matrix instructions (a k-ordered fmaf chain), correctly rounded square root / division in
 *     the clip + Adam step -- in EVERY form of it since round 6, including the reference's own [64,64] shape, whose handle applies Adam inside the next train kernel's
 *     prologue (or, with minibatches of <= 64 rows, inside the resident epoch kernel) during ppo_update.  No stated deviation is left in the default build.
 *     PPO_HIP_ADAM_FAST=1 (read at ppo_create) opts a handle into the hardware's 1-ulp reciprocal and square root for the quotient m * alpha / (sqrt(v) + eps) in ALL its
 *     Adam steps (a 3-ulp error in an update term that is ~1e-3 of the weight; 5 - 9 % of that shape's train step: bench.py reports both);
 *     PPO_HIP_NO_LAZY_ADAM=1 switches the deferred / resident forms themselves off.
 */
#ifndef PPO_HIP_H
#define PPO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPO_MAX_LAYERS 8
#define PPO_MAX_COMPONENTS 16
#define PPO_ABI_VERSION 3

typedef struct ppo_handle ppo_handle;

/* Everything the reference bakes into the graph file at generation time (SURVEY section 5 'config'):
 * network shape, ent_coef G:11323, vf_coef G:11395, max_grad_norm G:24370, Adam beta1/beta2/eps G:30430-30490. */
typedef struct ppo_config {
    int32_t obs_dim;                  /* O */
    int32_t act_dim;                  /* A */
    int32_t n_hidden;                 /* L, 1..PPO_MAX_LAYERS */
    int32_t hidden[PPO_MAX_LAYERS];   /* h0..h{L-1} */
    float ent_coef;
    float vf_coef;
    float max_grad_norm;
    float adam_beta1;
    float adam_beta2;
    float adam_eps;
    int32_t device;                   /* HIP device ordinal, -1 = current/LOCAL_RANK */
    int32_t max_rows;                 /* largest row count ever passed to step/value/train_step (0 = 65536) */
    int32_t compute_dtype;            /* PPO_F32 (0, default): the reference's arithmetic on the exact-fp32 matrix cores.
                                         PPO_BF16 (1): bf16 operands, fp32 accumulation, fp32 master weights / Adam, layer-by-layer
                                         128x128-tile GEMMs -- BASELINE configs[4]'s mode for wide nets; no reference counterpart */
} ppo_config;
#define PPO_F32 0
#define PPO_BF16 1

/* fills the graph-baked defaults of the reference's shipped graph (ent 0.00071602932, vf 0.5, clip 0.5,
 * Adam 0.9 / 0.999 / 1e-5) for the given shape */
void ppo_config_default(ppo_config* cfg, int32_t obs_dim, int32_t act_dim, int32_t n_hidden, const int32_t* hidden);

/* ---- lifecycle: SessionCreator::load_graph + Session::Run("init") (ppo2/session_creator.hpp:23-66) ---- */
/* ppo_create = ppo_create_ex(cfg, PPO_ACT_GAUSSIAN, out): the diagonal-Gaussian head (pi/logstd, a = mu + sigma * eps). */
int ppo_create(const ppo_config* cfg, ppo_handle** out);
/* Action distribution of the policy head (the reference's Env::get_action_space, env/env.hpp:51-56):
 *   PPO_ACT_GAUSSIAN     SPACE_CONTINOUS: cfg->act_dim = action dimensions
 *   PPO_ACT_CATEGORICAL  SPACE_DISCRETE: cfg->act_dim = number of categories A >= 2 (stable-baselines' CategoricalProbabilityDistribution:
 *                        logits l = h_L W_pi + b_pi, a = argmax_j (l_j - log(-log u_j)), neglogp = softmax cross-entropy against one_hot(a)).
 *                        An action is ONE float per row holding the category index ("categorical handle" below).  With PPO_F32 it runs the
 *                        generic fp32 kernel families.  With PPO_BF16 it needs the flag PPO_ACT_BF16_HEAD below; without the flag
 *                        that combination is refused.  Errors: act_dim < 2, an unknown action_dist, PPO_BF16 without PPO_ACT_BF16_HEAD, PPO_BF16 with
 *                        more than 128 categories.
 * Flags may be OR-ed into action_dist:
 *   PPO_ACT_SHAPE_KERNELS  PPO_ACT_CATEGORICAL | PPO_ACT_SHAPE_KERNELS lets a categorical PPO_F32 handle take the narrow LDS-resident family when its
 *                        shape qualifies as a Gaussian handle's would (every hidden width <= 64, padded observation and category widths <= 64, the
 *                        image fits 160 KB, PPO_HIP_NO_NARROW unset): one policy-step launch per env step ("narrow_step_kernel<cat>",
 *                        "narrow_step_kernel<cat,mask>") and narrow_train_kernel<cat[,mask]> + narrow_reduce_kernel + adam_kernel per train step.  A
 *                        shape that does not qualify runs the generic categorical kernels, as without the flag.  With PPO_ACT_GAUSSIAN the flag is
 *                        accepted and changes nothing.  Not the default (opt-in); data parallel is not available to such a handle: ppo_dist_init
 *                        refuses it.  ppo_action_dist reports the low bits only.
 *   PPO_ACT_BF16_HEAD    PPO_ACT_CATEGORICAL | PPO_ACT_BF16_HEAD with compute_dtype PPO_BF16 creates a categorical handle on the bf16 path: the GEMMs, the
 *                        head kernel, the backward chain, the weight-gradient GEMM and the assembly are the Gaussian handle's; the logits are the head's
 *                        fp32 partial products added in range order, and bf16_sample_kernel / bf16_loss_kernel run their <cat> / <cat,mask> forms (one
 *                        wave per row, lane l owns categories l and l + 64) with the arithmetic stated under "action masks of the categorical head"
 *                        below.  At most 128 categories: act_dim > 128 is an error of ppo_create_ex that names the limit.  Action masks, the masked
 *                        rollout and ppo_update work as on a PPO_F32 categorical handle.  ppo_kernel_counts names, counted INSTEAD of
 *                        "bf16_step_sequence" / "bf16_train_sequence": "bf16_step_sequence<cat>", "bf16_step_sequence<cat,mask>",
 *                        "bf16_train_sequence<cat>", "bf16_train_sequence<cat,mask>".  The tensor list has 4L+4 entries (no pi/logstd); the padded
 *                        logstd region keeps its place and is never moved.  With PPO_F32, or with PPO_ACT_GAUSSIAN, the flag is accepted and changes
 *                        nothing (same bits, same ppo_kernel_counts); PPO_ACT_SHAPE_KERNELS beside it on a PPO_BF16 handle is accepted and ignored (a
 *                        PPO_BF16 handle is never narrow).  Not the default (opt-in); data parallel is not available to such a handle: ppo_dist_init
 *                        refuses it ("... not supported for a categorical PPO_BF16 handle created with PPO_ACT_BF16_HEAD") and leaves it usable.
 *   PPO_ACT_PAIR_KERNELS PPO_ACT_CATEGORICAL | PPO_ACT_PAIR_KERNELS lets a categorical PPO_F32 handle take the [256,256] kernel pair when its shape qualifies as a
 *                        Gaussian handle's would (not wide, two hidden layers of 256, padded observation and category widths <= 64 -- at most 64 categories):
 *                        train8_kernel<cat[,mask]> + weight_grad_assemble_kernel + adam_kernel per train step instead of the generic four launches.  The head's
 *                        arithmetic is train_fwd_bwd_kernel<cat[,mask]>'s, stated under "action masks of the categorical head" below, in train8_kernel's geometry
 *                        (32 lanes per row; lane j owns categories j and j + 32): the d logits go where the Gaussian handle's d mu goes, the d logstd tile and
 *                        slot words are zeros, and the padded logstd region of the weights, the gradient and both Adam slots is never moved.  A row of ones as
 *                        mask gives the unmasked bits.  The act side is unchanged (policy_step_kernel<cat[,mask]>), and so are the epoch gather, ppo_update's
 *                        captured graph (kernel nodes only) and the Adam launch.  ppo_kernel_counts names, counted INSTEAD of "train8_kernel":
 *                        "train8_kernel<cat>", "train8_kernel<cat,mask>"; "weight_grad_assemble_kernel" keeps its one name.  PPO_HIP_NO_T8 and PPO_HIP_NO_DW2
 *                        act exactly as on a Gaussian handle: with PPO_HIP_NO_T8=1 the handle runs train_fwd_bwd_kernel<cat[,mask]> in front of
 *                        weight_grad_assemble_kernel (minibatches that are whole 64-row chunks), with PPO_HIP_NO_DW2=1 train8_kernel<cat[,mask]> in front of
 *                        weight_grad_kernel + grad_reduce_kernel.  A shape that does not qualify runs the generic categorical kernels, as without the flag
 *                        (same bits, same ppo_kernel_counts); with PPO_ACT_GAUSSIAN, with PPO_BF16, or beside PPO_ACT_SHAPE_KERNELS on a narrow shape the flag
 *                        is accepted and changes nothing.  A multi-categorical handle takes the pair through ppo_create_multi_ex's flag of the same name (below).  Not the
 *                        default (opt-in); data parallel is not available to a handle on which the flag took effect: ppo_dist_init refuses it ("... not
 *                        supported for a categorical handle created with PPO_ACT_PAIR_KERNELS") and leaves it usable.  ppo_action_dist reports the low bits only. */
#define PPO_ACT_GAUSSIAN    0
#define PPO_ACT_CATEGORICAL 1
#define PPO_ACT_SHAPE_KERNELS 0x100
#define PPO_ACT_BF16_HEAD 0x200
#define PPO_ACT_PAIR_KERNELS 0x400
int ppo_create_ex(const ppo_config* cfg, int32_t action_dist, ppo_handle** out);
int ppo_action_dist(const ppo_handle* h);          /* PPO_ACT_GAUSSIAN, PPO_ACT_CATEGORICAL, PPO_ACT_MULTI_CATEGORICAL or PPO_ACT_MULTI_BINARY */
/* ---- multi-categorical head: several independent choices per step (stable-baselines' MultiCategoricalProbabilityDistribution; env side: a multi-discrete space) ----
 * K components over ONE logits vector l = h_L W_pi + b_pi of width A = cfg->act_dim = n_0 + .. + n_{K-1}; component k owns columns S_k = [o_k, o_k + n_k), o_k the
 * running sum of the widths before it.  Tensor list, flat vector, orthogonal init and checkpoint tensors are those of a categorical handle with act_dim = A (4L+4
 * tensors, no pi/logstd).  An action is K floats per row, column k = the index WITHIN component k, in [0, n_k): every buffer that holds action rows is K wide
 * (ppo_step / ppo_act_deterministic [n,K], ppo_train_step actions [n,K], ppo_rollout_act actions_out [E,K], rollout field 1 [T,E,K]).  Noise stays [n,A] uniforms,
 * column j perturbs logit j; the counter draw stays keyed by (seed, global row, call counter, GLOBAL logit index j).  Per component, over its allowed set (all of it
 * when unmasked), the arithmetic is the categorical head's:
 *   sample a_k = argmax_{j in S_k} (l_j - log(-log u_j)) - o_k (lowest index on a tie), deterministic a_k = argmax_{j in S_k} l_j - o_k,
 *   m_k = max l_j, z_k = sum exp(l_j - m_k), neglogp_k = log z_k - (l_{a_k} - m_k), H_k = sum p_j (log z_k - (l_j - m_k));
 *   neglogp = sum_k neglogp_k and entropy = sum_k H_k, added in component order starting from the first component's value; the surrogate, value loss, approxkl and
 *   clipfrac see the row's total neglogp;  d logits_j = d_nlp (p_j - [j == o_k + a_k]) + ent_coef g p_j (log p_j + H_k) with H_k of j's OWN component.
 * A handle with ONE component nvec = {A} gives the SAME BITS as a PPO_ACT_CATEGORICAL handle with act_dim = A in every output.
 * Masks are [n, A] as for the categorical head and exclude per component; a row of ones gives the unmasked bits.  The host checks (before anything is uploaded;
 * each message names row and component): every COMPONENT of every mask row allows a category; a ppo_train_step_masked row's action k is allowed by its
 * component's mask; every action value of ppo_train_step / of an uploaded rollout field 1 is an integer in [0, n_k).
 * Runs the generic PPO_F32 kernel family (the narrow family, the [256,256] train8 pair and the bf16 path only through ppo_create_multi_ex's flags, below).  ppo_kernel_counts names,
 * counted INSTEAD of the <cat> ones: "policy_step_kernel<mcat>", "policy_step_kernel<mcat,mask>", "train_fwd_bwd_kernel<mcat>", "train_fwd_bwd_kernel<mcat,mask>".
 * Data parallel and both shuffles work as for a categorical PPO_F32 handle.
 * Errors of ppo_create_multi, each naming the limit: n_components outside 1..PPO_MAX_COMPONENTS, a component with fewer than 2 categories, cfg->act_dim != sum of
 * nvec, compute_dtype PPO_BF16 (without ppo_create_multi_ex's PPO_ACT_BF16_MULTI_HEAD).  ppo_create_ex(cfg, PPO_ACT_MULTI_CATEGORICAL, ..) stays an "unknown action_dist" error: the table has to come with the call. */
#define PPO_ACT_MULTI_CATEGORICAL 2
int ppo_create_multi(const ppo_config* cfg, const int32_t* nvec, int32_t n_components, ppo_handle** out);
/* ppo_create_multi with flags (ppo_create_multi(cfg, nvec, K, out) is ppo_create_multi_ex(cfg, nvec, K, 0, out): same checks, same messages, same bits).
 *   PPO_ACT_SHAPE_KERNELS  lets the handle take the narrow LDS-resident family under the rule of a flagged categorical handle: PPO_F32, every hidden width <= 64,
 *                        at most 4 hidden layers, padded observation and logit widths <= 64 (so sum of nvec <= 64), the image fits 160 KB, PPO_HIP_NO_NARROW
 *                        unset.  Then step, deterministic act, value, train step, update, rollout (device env and host Env, copy form, [E, K] action rows),
 *                        masks and the truncation bootstrap run narrow_step_kernel<mcat[,mask]> (one launch per env step) and
 *                        narrow_train_kernel<mcat[,mask]> + narrow_reduce_kernel + adam_kernel per train step, with the arithmetic stated above per component.
 *                        One component gives the bits of a flagged categorical handle; a row of ones as mask gives the unmasked bits; the same seed draws what
 *                        the generic <mcat> kernels draw.  ppo_kernel_counts names, counted INSTEAD of the <cat> and the generic names:
 *                        "narrow_step_kernel<mcat>", "narrow_step_kernel<mcat,mask>", "narrow_train_kernel<mcat>", "narrow_train_kernel<mcat,mask>".  A shape
 *                        that does not qualify runs the generic <mcat> kernels, as without the flag (data parallel included).  Not the default (opt-in).
 *                        Measured at (18, (6, 6, 6), [64,64]): train step 0.76 / 0.71 of the generic one's time at 64 / 2048 rows, policy step 0.90 / 0.95 at
 *                        16 / 1024 rows; it lost at no row count measured.  A shape whose plain image exceeds 160 KB takes a compact tile layout.
 *                        Data parallel is not available to a handle on which the flag took effect: ppo_dist_init refuses it ("... not supported for a
 *                        multi-categorical handle created with PPO_ACT_SHAPE_KERNELS") and leaves it usable.
 *   PPO_ACT_PAIR_KERNELS   lets the handle take the [256,256] kernel pair under the rule of a flagged categorical handle: PPO_F32, not wide, two hidden layers
 *                        of 256, padded observation and logit widths <= 64 (so sum of nvec <= 64).  A train step then runs train8_kernel<mcat[,mask]> +
 *                        weight_grad_assemble_kernel + adam_kernel instead of the generic four launches, with the arithmetic stated above per component in
 *                        train8_kernel's geometry (32 lanes per row; lane j owns logit columns j and j + 32, which may belong to two components; a row's K
 *                        action indices wait in a region of their own behind the other instantiations' LDS carve).  The d logits go where d mu goes, the
 *                        d logstd tile and slot words are zeros, and the padded logstd region of the weights, the gradient and both Adam slots is never moved.
 *                        One component gives the bits of a categorical handle created with PPO_ACT_PAIR_KERNELS; a row of ones as mask gives the unmasked
 *                        bits.  The act side is unchanged (policy_step_kernel<mcat[,mask]>), and so are the epoch gather ([.., K] action rows), the masked
 *                        rollout, the truncation bootstrap, ppo_update's captured graph (kernel nodes only) and the Adam launch.  ppo_kernel_counts names,
 *                        counted INSTEAD of "train_fwd_bwd_kernel<mcat>" / "train_fwd_bwd_kernel<mcat,mask>": "train8_kernel<mcat>",
 *                        "train8_kernel<mcat,mask>"; "weight_grad_assemble_kernel" keeps its one name.  PPO_HIP_NO_T8 and PPO_HIP_NO_DW2 act as on a flagged
 *                        categorical handle: with PPO_HIP_NO_T8=1 train_fwd_bwd_kernel<mcat[,mask]> in front of weight_grad_assemble_kernel (minibatches that
 *                        are whole 64-row chunks), with PPO_HIP_NO_DW2=1 train8_kernel<mcat[,mask]> in front of weight_grad_kernel + grad_reduce_kernel.  A
 *                        shape that does not qualify runs the generic <mcat> kernels, as without the flag (same bits, same ppo_kernel_counts, data parallel
 *                        included).  Beside PPO_ACT_SHAPE_KERNELS the two rules never both hold (hidden widths <= 64 against two layers of 256): each flag
 *                        acts where its own rule holds.  Not the default (opt-in).  Measured at (18, (6, 6, 6), [256,256]) against the unflagged handle in one process: train step 40.9 against 50.1 us at 64 rows (0.82) and
 *                        49.7 against 58.1 us at 2048 rows (0.85), beside 39.6 / 49.3 us for train8_kernel<cat> at act_dim = 18; at (50, (4,) x 16), K = 16, 52.4
 *                        against 74.8 and 62.2 against 88.3 us (0.70), 9 us above train8_kernel<cat> at 64 categories: the component walk costs about half a
 *                        microsecond per component.  It lost to the generic form at no row count measured.
 *                        Data parallel is not available to a handle on which the flag took effect: ppo_dist_init refuses it ("... data parallel is not
 *                        supported for a multi-categorical handle created with PPO_ACT_PAIR_KERNELS") and leaves it usable.
 *   PPO_ACT_BF16_HEAD    accepted, nothing to select (the flag belongs to ppo_create_ex's categorical head; this head's bf16 forms are asked for with
 *                        PPO_ACT_BF16_MULTI_HEAD); compute_dtype PPO_BF16 stays refused with it.
 *   PPO_ACT_BF16_MULTI_HEAD  with compute_dtype PPO_BF16 creates the handle on the bf16 path (wide nets): staging, the hidden-layer GEMMs, bf16_heads_kernel, the
 *                        backward links, the weight-gradient GEMM and the assembly + clip + Adam launch are those of every PPO_BF16 handle; the logits are the head
 *                        GEMM's fp32 partial products added in range order, and bf16_sample_kernel / bf16_loss_kernel run their <mcat> / <mcat,mask> forms: one
 *                        wave per row, lane l owns logits l and l + 64 (so sum of nvec <= 128; more is an error that names the limit), and the lanes walk the K
 *                        components with the arithmetic stated above, 64-lane butterflies per component ("none yet" of a masked component = one past its end).
 *                        The d logits go where d mu goes (forbidden and padding columns exactly +0), the d logstd slot words are zeros.  One component gives the
 *                        bits of a categorical PPO_BF16 handle (PPO_ACT_BF16_HEAD) in every output; a row of ones as mask gives the unmasked bits; the act
 *                        model's neglogp is the train model's.  Every entry point of a multi-categorical handle works: step / act (masked too), train step,
 *                        the rollout calls with ppo_set_action_masking and field 8, ppo_update (kernel nodes only in its captured graph), ppo_collect_synthetic,
 *                        ppo_get_last_grad, checkpoints (the tensors of an fp32 handle of the same nvec).  PPO_HIP_NO_BF16_CHAIN and PPO_HIP_NO_REDUCE_ADAM act
 *                        as on every PPO_BF16 handle.  ppo_kernel_counts names, counted INSTEAD of "bf16_step_sequence" / "bf16_train_sequence":
 *                        "bf16_step_sequence<mcat>", "bf16_step_sequence<mcat,mask>", "bf16_train_sequence<mcat>", "bf16_train_sequence<mcat,mask>".  Without
 *                        the flag PPO_BF16 stays refused; with PPO_F32 the flag is accepted and changes nothing (same bits, same ppo_kernel_counts);
 *                        PPO_ACT_SHAPE_KERNELS / PPO_ACT_PAIR_KERNELS beside it on a PPO_BF16 handle are accepted and ignored.  ppo_create_ex rejects the bit.
 *                        Measured at (256 observations, [1024,1024,1024], nvec = (16,) x 4) against the generic fp32 <mcat> handle in one process: train step 242.1
 *                        against 1275.8 us at 4096 rows (0.19) and 170.8 against 524.5 us at 256 rows, policy step 153.2 against 850.9 us at 8192 rows; with 128 logits
 *                        the generic family cannot hold that net.  Sixteen components cost 1.09 of the categorical PPO_BF16 handle's train step and 1.36 of its policy
 *                        step: about 1.7 us per component of dependent butterflies.
 *                        Not the default (opt-in).  Data parallel is not available: ppo_dist_init refuses the handle ("... data parallel is not supported for a
 *                        multi-categorical PPO_BF16 handle created with PPO_ACT_BF16_MULTI_HEAD") and leaves it usable.
 * Any other bit is an error ("ppo_create_multi_ex: unknown flag bit 0x.."). */
#define PPO_ACT_BF16_MULTI_HEAD 0x1000
int ppo_create_multi_ex(const ppo_config* cfg, const int32_t* nvec, int32_t n_components, int32_t flags, ppo_handle** out);
/* the handle's component widths: returns K and fills at most `max` entries; 0 for a Gaussian or multi-binary handle, 1 with nvec[0] = A for a categorical one */
int ppo_action_nvec(const ppo_handle* h, int32_t max, int32_t* nvec);
/* columns of one action row: A (Gaussian, multi-binary), 1 (categorical) or K (multi-categorical) */
int ppo_action_width(const ppo_handle* h);
/* Multi-binary action spaces (stable-baselines' BernoulliProbabilityDistribution over MultiBinary(A)): ppo_create_ex(cfg, PPO_ACT_MULTI_BINARY, out), A = cfg->act_dim
 * >= 1 independent on / off decisions per step over the logits l = h_L W_pi + b_pi of width A.  (The name is multi_binary everywhere; "bernoulli" is no action_dist.)
 *   Tensors: a categorical handle's 4L+4 (no pi/logstd; the padded logstd region of weights, gradient and both Adam slots keeps its place and is never moved).
 *   Actions: A floats per row, each exactly 0 or 1: ppo_action_width = A, every buffer that holds action rows has the Gaussian handle's shape; ppo_action_dist = 3,
 *   ppo_action_nvec = 0.  Noise: [n, A] uniforms in [0, 1), as for the categorical head; without explicit noise column j draws ctr_uniform(seed, row, step, j) under the
 *   categorical head's keys.
 *   Per element, with e = exp(-|l|), sp = log1p(e), q = e / (1 + e) (ppo_head.hpp: bern_parts, bern_nlp_elem, bern_entropy_elem, bern_grad_elem):
 *     p = l >= 0 ? 1 / (1 + e) : q;  sampled x = u < p ? 1 : 0;  deterministic x = l > 0 ? 1 : 0 (tf.round(sigmoid(l)): a logit of +-0 gives 0)
 *     neglogp_j = sp + (x_j == (l_j > 0) ? 0 : |l_j|)   (= TF's relu(l) - l x + log1p(exp(-|l|)));   H_j = sp + |l_j| q_j;   the row's neglogp and entropy: sums over j
 *     d loss / d l_j = d_nlp (p_j - x_j) + ent_coef g l_j p_j (1 - p_j), p (1 - p) = e / (1 + e)^2; padding columns and dead rows get exactly +0; the aux (d logstd)
 *     words are zeros.  This is the derivative of the SMOOTH identity softplus(l) - l x: at a logit of exactly +-0 TensorFlow's composed graph (and autograd of the
 *     literal relu / abs expression) differentiates the kinks to 0 and gives another value there.
 *   Surrogate, value loss, approxkl and clipfrac see the row's neglogp unchanged.  float32 against float64 at 4096 x 18 logits: neglogp within 3.0e-6 abs at a spread
 *   of +-1.5, 9e-7 at +-40, 5e-7 at +-120; entropy within 3.0e-6 / 5e-7 / 2e-7; nothing overflows.
 *   Without PPO_ACT_BINARY_SHAPE_KERNELS or PPO_ACT_BINARY_PAIR_KERNELS (below) the handle runs the generic fp32 family ("policy_step_kernel<mbin>" / "train_fwd_bwd_kernel<mbin>" in ppo_kernel_counts,
 *   instead of the plain names) on any hidden widths: never narrow, never train8_kernel, deferred Adam, the resident epoch kernel or a one-launch rollout -- the rules
 *   of an unflagged categorical handle.
 *   PPO_ACT_SHAPE_KERNELS, PPO_ACT_PAIR_KERNELS and PPO_ACT_BF16_HEAD beside it on a PPO_F32 handle are accepted and change nothing (same bits, same counts).
 *   Every entry point of a categorical PPO_F32 handle works, actions [., A]; data parallel (ppo_dist_init, both shuffles) included.
 *   Host checks before anything is uploaded: every action of ppo_train_step / ppo_rollout_upload field 1 is exactly 0 or 1 (the message names row and column; NaN is
 *   refused); the masked entry points and ppo_set_action_masking refuse the handle ("action masks need a categorical ...").
 *   Errors of ppo_create_ex, each naming the limit: act_dim < 1; compute_dtype PPO_BF16.  2 stays an "unknown action_dist" error, as does 3 with an unknown flag bit.
 *   Measured on an MI355X (us of device time per call at 18 obs, hidden [256,256]; this head | a categorical handle of 18 categories | a
 *   multi-categorical one with nvec = (2,) x 16): policy step 16.6 | 16.5 | 29.1 at 16 rows, 17.6 | 18.6 | 29.7 at 1024; train_fwd_bwd_kernel 25.5 | 24.3 | 39.4 at 64 rows,
 *   26.6 | 26.0 | 40.4 at 2048.  The elementwise head is about 1 us SLOWER than <cat> per train launch; it has not been tuned.
 *   Out of scope for this head: the bf16 path, the fused host step and the resident rollouts, action masks.
 *   PPO_ACT_BINARY_SHAPE_KERNELS  PPO_ACT_MULTI_BINARY | PPO_ACT_BINARY_SHAPE_KERNELS lets a multi-binary PPO_F32 handle take the narrow LDS-resident family's step and
 *                        train kernels under the rule of a flagged categorical handle: at most 4 hidden layers, every padded hidden width <= 64, padded
 *                        observation and action widths <= 64, the plain LDS image within 160 KB, PPO_HIP_NO_NARROW unset.  (A flag of its own: PPO_ACT_SHAPE_KERNELS
 *                        on this head is accepted and changes nothing, and stays so.)  Same arithmetic per element as the generic <mbin> kernels, the same counter
 *                        keys: the same seed and rows draw what the generic kernels draw wherever u is not within rounding of p.  ppo_kernel_counts_all names,
 *                        counted INSTEAD of the generic <mbin> names: "narrow_step_kernel<mbin>", "narrow_train_kernel<mbin>" (static and runtime shapes share a
 *                        name; the form launched under ppo_set_target_kl counts as the train kernel).  A train step is that launch + narrow_reduce_kernel +
 *                        adam_kernel; no deferred Adam, no resident epoch, no one-launch rollout: ppo_set_host_step_fused and ppo_set_rollout_resident are
 *                        accepted and change nothing (per-step launches on the device env, the copy form behind a host Env).  Masks and PPO_BF16 stay refused, the
 *                        0 / 1 action checks stay.  A shape that does not qualify runs the generic <mbin> kernels, as without the flag (same bits, same counts, data
 *                        parallel included).  Where the flag took effect ppo_dist_init refuses ("... data parallel is not supported for a multi-binary handle
 *                        created with PPO_ACT_BINARY_SHAPE_KERNELS") and leaves the handle usable.  With any other distribution the bit is an "unknown
 *                        action_dist" error, whose text names it; ppo_create_multi_ex refuses it with its own "unknown flag bit 0x2000".
 *   PPO_ACT_BINARY_PAIR_KERNELS  PPO_ACT_MULTI_BINARY | PPO_ACT_BINARY_PAIR_KERNELS lets a multi-binary PPO_F32 handle take the [256,256] train kernel pair under the
 *                        rule of a categorical handle created with PPO_ACT_PAIR_KERNELS: exactly two hidden layers of 256, padded observation and action widths
 *                        <= 64 (at most 64 observations and 64 bits).  (A flag of its own: PPO_ACT_PAIR_KERNELS on this head is accepted and changes nothing, and
 *                        stays so.)  A train step is train8_kernel<mbin> + weight_grad_assemble_kernel + adam_kernel: the Gaussian form's prologue, towers and
 *                        backward, the head block elementwise in the Gaussian form's lane geometry with exp / log1p formed once per element; d logits go where
 *                        d mu goes, the aux words are zeros and the padded logstd region of theta, Adam and the gradient is never touched.  The act side stays
 *                        policy_step_kernel<mbin>: step and deterministic actions give the bits of the unflagged handle.  Counted under "train8_kernel<mbin>"
 *                        INSTEAD of "train_fwd_bwd_kernel<mbin>" (the form launched under ppo_set_target_kl counts under the same name) -- a name of
 *                        ppo_kernel_count / ppo_kernel_variant_name only -- and "weight_grad_assemble_kernel" as on every pair handle.  PPO_HIP_NO_T8 /
 *                        PPO_HIP_NO_DW2 act as on a flagged categorical handle: one set, half the pair runs; both set, the flag did not take effect.  Masks and
 *                        PPO_BF16 stay refused, the 0 / 1 action checks stay.  A shape that does not qualify runs the generic <mbin> kernels, as without the flag
 *                        (same bits, same counts, data parallel included); beside PPO_ACT_BINARY_SHAPE_KERNELS each flag takes effect on its own shape.  Where the
 *                        flag took effect ppo_dist_init refuses ("ppo_dist_init: data parallel is not supported for a multi-binary handle created with
 *                        PPO_ACT_BINARY_PAIR_KERNELS (create it without the flag)") and leaves the handle usable.  With any other distribution the bit is an
 *                        "unknown action_dist" error, whose text names it; ppo_create_multi_ex refuses it with its own "unknown flag bit 0x4000".
 *                        Measured on an MI355X at (18 obs, 18 bits, [256,256]) against the unflagged handle of the same run (us of device
 *                        time per call): train step 40.3 against 49.5 at 64 rows, 49.6 against 57.2 at 2048; the policy step runs the same kernel (16.8 | 16.5 at
 *                        16 rows, 18.0 | 17.8 at 1024). */
#define PPO_ACT_MULTI_BINARY 3
#define PPO_ACT_BINARY_SHAPE_KERNELS 0x2000
#define PPO_ACT_BINARY_PAIR_KERNELS 0x4000
void ppo_destroy(ppo_handle* h);
const char* ppo_last_error(const ppo_handle* h);   /* h may be NULL: error of the last failed ppo_create */
int ppo_abi_version(void);

/* ---- variables: initializer consts G:2249-5297 / saver G:32312-33437 (ppo2/ppo2.hpp:107-223) ----------
 * Tensors are addressed by index in TF trainable-variable order
 *   pi_fc0/w, pi_fc0/b, vf_fc0/w, vf_fc0/b, pi_fc1/w, ... , vf/w, vf/b, pi/w, pi/b, pi/logstd   (4L+5 tensors)
 * A categorical handle has no pi/logstd (4L+4 tensors; pi/w is [h_last, A], pi/b [A]); the flat vector and ppo_get_last_grad follow. 
 * `which`: 0 = weights, 1 = Adam m slot, 2 = Adam v slot. */
int ppo_num_tensors(const ppo_handle* h);
int ppo_tensor_info(const ppo_handle* h, int index, char name[32], int32_t* rows, int32_t* cols); /* cols 0 = 1-D */
int ppo_num_params(const ppo_handle* h);                      /* dense count (146213 for 18/18/[256,256]) */
int ppo_get_tensor(ppo_handle* h, int which, int index, float* dst, int64_t count);
int ppo_set_tensor(ppo_handle* h, int which, int index, const float* src, int64_t count);
/* dense flat vector in the order above (the layout of the oracle's theta / m / v) */
int ppo_get_flat(ppo_handle* h, int which, float* dst, int64_t count);
int ppo_set_flat(ppo_handle* h, int which, const float* src, int64_t count);
int ppo_get_beta_powers(ppo_handle* h, float pw[2]);          /* beta1_power, beta2_power (G:25426,25579) */
int ppo_set_beta_powers(ppo_handle* h, const float pw[2]);
/* orthogonal init of the same family as the constants in G (gain sqrt2 hidden, 0.01 pi, 1.0 vf; biases,
 * logstd, Adam slots zero; beta powers = beta) */
int ppo_init_orthogonal(ppo_handle* h, uint64_t seed);
/* seed of the on-device action-noise generator that stands in for G:5894 RandomStandardNormal when no explicit noise
 * is passed (the reference seeds TF from the clock, ppo2.cpp:159-162; PPO2::seed / --seed end up here).  The draw for
 * a row is keyed by (seed, global row = rank * n_envs + row, call counter, action index), so data-parallel ranks
 * draw independent noise. */
int ppo_seed(ppo_handle* h, uint64_t seed);

/* ---- act model ------------------------------------------------------------------------------------------
 * MlpPolicy::step (ppo2/policies.hpp:33-46): feeds input/Ob:0, fetches output/_action, _value_flat, _neglogp.
 * noise [n,A] = the N(0,1) draw of G:5894 made explicit (parity mode); NULL = on-device counter RNG.
 * Categorical handle: action [n] (category indices); noise [n,A] = the uniforms u in [0,1) of the Gumbel-argmax draw, NULL = an on-device
 * counter draw in (0,1) keyed like the Gaussian's (seed, global row, call counter, category).  ppo_act_deterministic writes argmax_j l_j [n]. */
int ppo_step(ppo_handle* h, const float* obs, int32_t n, const float* noise, float* action, float* value,
             float* neglogp);
/* MlpPolicy::value (ppo2/policies.hpp:64-77) */
int ppo_value(ppo_handle* h, const float* obs, int32_t n, float* value);
/* MlpPolicy::get_deterministic_action (ppo2/policies.hpp:49-62) */
int ppo_act_deterministic(ppo_handle* h, const float* obs, int32_t n, float* action);

/* ---- querying the policy: given actions and the action distribution (no reference counterpart: its MlpPolicy fetches action, value_flat, neglogp and
 * deterministic_action only; stable-baselines 2 ActorCriticPolicy.proba_step / BaseRLModel.action_probability, stable-baselines 3 evaluate_actions) -------------
 * All three run policy_eval_kernel: the act model's two towers on policy_step_kernel's geometry, no random draw, the head arithmetic of
 * ppo_head.hpp.  Every PPO_F32 handle runs this one generic kernel -- also a handle whose step runs the narrow family (its results then agree with ppo_step's to
 * rounding, not bit for bit; on a handle whose step runs policy_step_kernel neglogp and value are ppo_step's bits).  A PPO_BF16 handle is refused: its step's neglogp
 * comes out of bf16 GEMMs and an fp32 evaluation would disagree with it (a bf16 form is future work).  A data-parallel handle evaluates its own rows, no collective.
 * The calls are STATELESS: they do not advance the counter RNG and touch neither rollout, normaliser nor Adam state; they are legal in the middle of a rollout on
 * every rollout form (a resident rollout kernel is retired and relaunched as for ppo_value) and see the weights of the last finished ppo_update / ppo_train_step.
 * One exception to "one launch, nothing written but the outputs": on a handle whose step runs the narrow family, the train forms keep the weights and the packed
 * image current but not the small-parameter mirror ("par") and the transposed copies ("thetaT") that only the generic kernels read.  The first query behind a
 * ppo_train_step / ppo_update on such a handle therefore launches transpose_refresh_kernel once in front of its own kernel: both buffers are rewritten from the
 * weights -- derived copies, no weight, Adam slot or random state changes, and no narrow kernel reads them.  That launch is not counted by ppo_kernel_counts either and
 * is not timed under a ppo_prof_read class.
 * They are NOT counted by ppo_kernel_counts (its rows and every count stay what they were); ppo_prof_read books them under "policy_step".  (In the middle of a
 * rollout that a resident kernel serves, the relaunch of that kernel behind the query is counted like every launch of it, as behind ppo_value.)
 *   ppo_distribution_width  W, the columns of one parameter row: Gaussian 2A (mu[0..A) | std[0..A)), categorical A (probabilities), multi-categorical sum(nvec)
 *                           (each component's probabilities, in logit order), multi-binary A (P(bit = 1)).
 *   ppo_evaluate_actions    obs [n,O] as ppo_step takes them, actions [n, ppo_action_width] as ppo_train_step takes them, mask NULL or [n,A] as ppo_step_masked takes
 *                           it; value / neglogp / entropy each [n] or NULL, not all NULL.  neglogp is that of the GIVEN action, entropy the row's.  Host checks
 *                           before anything is uploaded, as for ppo_train_step[_masked]: a categorical index is an integer in [0, A) (per component [0, n_k)), a
 *                           bit is 0 or 1, a mask row (component) allows a category and its own action; a mask on a Gaussian or multi-binary handle is refused.
 *   ppo_action_probability  params [n,W], count = n * W.  A forbidden category's probability is exactly +0.
 *   ppo_rollout_evaluate    the same kernel straight on the device-resident rollout -- fields 0 (obs), 1 (actions) and, on a masking handle, 8 (masks): T*E rows in
 *                           time-major order, nothing staged from the host -- each output [T,E] or NULL, not all NULL.  Needs a FINISHED rollout (ppo_rollout_finish /
 *                           ppo_collect_synthetic since the last ppo_rollout_alloc / ppo_rollout_act); otherwise an error.  After ppo_update: the true neglogp, entropy
 *                           and value of the batch just trained on under the new weights.
 * A refusal launches nothing and leaves the handle usable.  n has ppo_step's limits. */
int ppo_distribution_width(const ppo_handle* h);
int ppo_evaluate_actions(ppo_handle* h, const float* obs, const float* actions, int32_t n, const float* mask, float* value, float* neglogp,
                         float* entropy);
int ppo_action_probability(ppo_handle* h, const float* obs, int32_t n, const float* mask, float* params, int64_t count);
int ppo_rollout_evaluate(ppo_handle* h, float* value, float* neglogp, float* entropy);

/* ---- action masks of the categorical head (invalid-action masking; no reference counterpart) ---------------
 * A mask is one float per (row, category), [n, A]: non-zero = allowed, 0 = forbidden.  For a masked row with logits l and allowed set S:
 *   forbidden categories are EXCLUDED, not pushed down by a constant:  m = max_{j in S} l_j,  z = sum_{j in S} exp(l_j - m),
 *   p_j = exp(l_j - m) / z for j in S, p_j = 0 otherwise
 *   sample         argmax_{j in S} (l_j - log(-log u_j)), lowest index on a tie.  The noise layout [n, A] and the counter draw's keys are unchanged:
 *                  forbidden categories still own their uniforms, a mask does not shift the draws of the others
 *   deterministic  argmax_{j in S} l_j
 *   neglogp        log z - (l_a - m)
 *   entropy        sum_{j in S} p_j (log z - (l_j - m))
 *   d logits       d_nlp (p_j - [j == a]) + ent_coef g p_j (log p_j + H) for j in S, exactly 0 otherwise: the pi/w columns and pi/b entries of a category
 *                  that is forbidden in every row of a minibatch receive a zero gradient
 *   a row of ones gives the SAME BITS as the unmasked kernels in every output (action, neglogp, value, losses, gradient, weights after Adam): the mask is
 *   read inside policy_step_kernel / train_fwd_bwd_kernel by the lane that owns the category, the lane loops and butterflies are the unmasked ones.
 * Errors, checked on the HOST before anything is uploaded (like the category-index check; nothing is trained): a row without an allowed category wherever
 * the mask comes from the host (the three calls below, ppo_rollout_act_masked, ppo_rollout_upload of field 8), and a ppo_train_step_masked row whose action
 * its own mask forbids.  ppo_update has no host check: if the rollout's action field was uploaded inconsistently with its mask field, the loss values of
 * such a row are unspecified (the kernels still read and write inside their buffers and terminate).
 * The three calls need a categorical or multi-categorical handle (a Gaussian handle, PPO_F32 or PPO_BF16: an error); mask == NULL is the unmasked call, the same launch. */
int ppo_step_masked(ppo_handle* h, const float* obs, int32_t n, const float* noise, const float* mask, float* action, float* value,
                    float* neglogp);
int ppo_act_deterministic_masked(ppo_handle* h, const float* obs, int32_t n, const float* mask, float* action);
int ppo_train_step_masked(ppo_handle* h, float lr, float cliprange, const float* obs, const float* actions, const float* mask,
                          const float* advs, const float* returns, const float* old_neglogp, const float* old_values, int32_t n,
                          float losses[5]);
/* Masks in the device-resident rollout: a handle setting (default off; turning it on is an error on a handle that is not categorical).  With it on,
 * ppo_rollout_alloc also allocates a [T, E, A] mask buffer initialised to ones, the epoch gather copies the mask rows into minibatch order beside the
 * other fields, and ppo_update runs the masked train kernel over them (ppo_kernel_counts: "policy_step_kernel<cat,mask>", "train_fwd_bwd_kernel<cat,mask>").
 * CHANGING the setting drops an allocated rollout (and the captured update): rollout calls report "no rollout allocated" until the next ppo_rollout_alloc.
 * A handle that never turns it on enqueues exactly the launches it enqueued before these entry points existed.  Data parallel: every rank masks and
 * gathers its own rows, nothing new crosses ranks; ppo_dist_global_shuffle(h, 1) together with masking is refused by ppo_update. */
int ppo_set_action_masking(ppo_handle* h, int on);
int ppo_get_action_masking(const ppo_handle* h);

/* ---- train op: PPO2::_train_step's Session::Run (ppo2/ppo2.hpp:430-468) ---------------------------------
 * feeds train_model/input/Ob, loss/{action,advs,rewards,old_neglog_pac,old_vpred,learning_rate,clip_range}_ph;
 * target ppo2/_train; losses = {pg_loss, vf_loss, entropy, approxkl, clipfrac}.  `advs` are ALREADY normalised
 * (the reference normalises on the host, ppo2/ppo2.hpp:401-406; ppo_adv_normalize does it on the device). */
int ppo_train_step(ppo_handle* h, float lr, float cliprange, const float* obs, const float* actions,
                   const float* advs, const float* returns, const float* old_neglogp, const float* old_values,
                   int32_t n, float losses[5]);
/* Categorical handle: actions [n], every value an integer in [0, A) (checked on the host before the upload: an error otherwise); the loss
 * is the same surrogate with the softmax cross-entropy as neglogp and the categorical entropy. */
/* value-function clipping: PPO2's cliprange_vf (ppo2/ppo2.hpp:442-446 feeds loss/clip_range_vf_ph, a node the shipped graph lacks).
 * Per row, with v the new value, vo the old value, R the return (vf_loss = 1/2 mean over rows, clipfrac stays the policy's):
 *   PPO_VCLIP_POLICY  max((v-R)^2, (vo + clip(v-vo, +-cliprange) - R)^2): the graph's own loss, bit for bit (the default)
 *   PPO_VCLIP_RANGE   the same with `range` (finite, >= 0) in place of cliprange
 *   PPO_VCLIP_OFF     (v-R)^2, unclipped
 * `range` is ignored in the other two modes.  The setting belongs to the handle and applies from the next ppo_train_step / ppo_update on
 * (a replayed update graph follows it: the kernels read it from device memory, as they read lr and cliprange).  An unknown mode or a
 * negative / NaN / infinite range in PPO_VCLIP_RANGE is an error that leaves the previous setting in place. */
#define PPO_VCLIP_POLICY 0
#define PPO_VCLIP_RANGE  1
#define PPO_VCLIP_OFF    2
int ppo_set_value_clip(ppo_handle* h, int32_t mode, float range);
/* the handle's current setting; range reads 0 outside PPO_VCLIP_RANGE */
int ppo_get_value_clip(const ppo_handle* h, int32_t* mode, float* range);
/* Target-KL early stopping (no reference counterpart; the knob stable-baselines3 and spinning-up call target_kl).  0 = off (the default).  With target_kl > 0:
 *   limit = 1.5f * target_kl, computed in fp32 on the host (stable-baselines3's factor).  The ESTIMATOR is the project's own approxkl -- losses[3], the graph's
 *   half mean squared log-ratio 1/2 mean((neglogp - old_neglogp)^2) -- NOT stable-baselines3's k3 estimator mean(exp(r) - 1 - r); the two agree to second order.
 *   Train step k of a ppo_update computes its losses and gradient as always, with the weights as they stand.  If approxkl_k > limit NOTHING of step k is applied:
 *   the weights, both Adam slots and the beta powers stay bit for bit as they were, and every later step of that update does nothing.  The comparison is taken on
 *   the device, inside the launch that applies the step, with the fp32 expression that writes the returned row: a host that compares loss_rows[k][3] against
 *   1.5f * target_kl reproduces it exactly.  (A NaN approxkl does not exceed the limit: such a step is applied, as it is with the setting off.)
 *   A stopped update returns loss_rows[0..k] as computed (the triggering row included), quiet NaN in every row behind k, mean_losses = the column means of rows
 *   0..k only; ppo_get_last_grad and its norm are those of step k.  The next ppo_update starts with the stop condition cleared (also when it replays the captured
 *   graph; a changed target_kl is honoured by a replay, switching between off and on re-captures).  ppo_train_step[_masked] follows the same rule for its single
 *   step: the losses are returned, the step is not applied when its approxkl exceeds the limit.
 *   Form selection: with the setting on, ppo_update takes the launch sequences that end every train step in adam_kernel -- what PPO_HIP_NO_LAZY_ADAM=1 +
 *   PPO_HIP_NO_NARROW_EPOCH=1 select (no narrow_epoch_kernel in ppo_kernel_counts); the narrow reference shape gives up its deferred Adam and resident epochs for it.
 *   With the setting off a handle enqueues exactly what it always did.
 *   Refused, with an error that leaves the handle usable and the previous setting in place: a negative, NaN or infinite value; target_kl > 0 on a PPO_BF16
 *   handle; target_kl > 0 on a handle with a communicator (and ppo_dist_init on a handle with the setting on). */
int ppo_set_target_kl(ppo_handle* h, float target_kl);
int ppo_get_target_kl(const ppo_handle* h, float* target_kl);
/* Adam steps applied / train steps enqueued by the last ppo_update or ppo_train_step[_masked] (applied == total with the setting off) */
int ppo_update_applied(ppo_handle* h, int32_t* applied, int32_t* total);
/* gradient of the last train step (of ppo_train_step, or the last one of ppo_update) BEFORE clipping (debug/parity), dense flat order.
 * PPO_BF16 handles on one GPU do not keep it: it is rebuilt here from the step's partial sums (same bits), which stay valid until the next train step. */
int ppo_get_last_grad(ppo_handle* h, float* dst, int64_t count, float* global_norm);

/* ---- fused host-loop numerics the north star moves onto the device ----------------------------------------
 * PPO2::_train_step prologue (ppo2/ppo2.hpp:401-406) */
int ppo_adv_normalize(ppo_handle* h, const float* returns, const float* values, int32_t n, float* advs);
/* Runner::set_returns (ppo2/runner.hpp:159-191); [T,E] time-major; last_dones = dones after the last step */
int ppo_gae(ppo_handle* h, const float* rewards, const float* values, const float* dones,
            const float* last_values, const float* last_dones, int32_t T, int32_t E, float gamma, float lam,
            float* returns);
/* The same scan with a value bootstrap at time-limit TRUNCATIONS (no reference counterpart: Runner::set_returns treats every done as a terminal state).
 * terminal_values [T,E]: V(terminal observation) on the rows whose step was cut by a time limit, 0 elsewhere.  The reward of a row becomes
 * rewards + gamma * terminal_values; the lambda trace is still cut at the episode boundary (stable-baselines3's rule):
 *   delta_t = (rewards[t] + gamma tv[t]) + gamma V[t+1] (1 - done[t+1]) - V[t]        (done[t+1]: row t+1 holds the done raised by step t; last_dones for t = T-1)
 * terminal_values == NULL is ppo_gae, bit for bit (the same launch). */
int ppo_gae_ex(ppo_handle* h, const float* rewards, const float* values, const float* dones, const float* last_values,
               const float* last_dones, const float* terminal_values, int32_t T, int32_t E, float gamma, float lam,
               float* returns);

/* EnvNormalize (env/env_normalize.hpp:20-116) + RunningStatistics (common/running_statistics.hpp). */
int ppo_norm_init(ppo_handle* h, int32_t n_envs, float gamma, float clip_obs, float clip_rew, float epsilon);
int ppo_norm_obs(ppo_handle* h, const float* raw_obs, int32_t n_envs, int training, float* out);
int ppo_norm_reward(ppo_handle* h, const float* raw_rew, const float* dones, int32_t n_envs, int training,
                    float* out);
/* the norm_obs / norm_reward constructor flags of EnvNormalize (env_normalize.hpp:24-27, honoured at :75 and :95): with
 * norm_obs == 0 observations pass through unscaled and obs_rms is never updated; with norm_reward == 0 rewards pass
 * through and ret_rms is never updated (the discounted return is still accumulated, :66).  Default 1, 1. */
int ppo_norm_set_flags(ppo_handle* h, int norm_obs, int norm_reward);
/* EnvNormalize::reset's `ret = Zero` (env_normalize.hpp:111-116) without touching the statistics */
int ppo_norm_reset_returns(ppo_handle* h);
/* which: 0 = obs_rms, 1 = ret_rms; serialise / deserialise of env_normalize.hpp:134-146 */
int ppo_norm_get_stats(ppo_handle* h, int which, float* mean, float* var, double* count);
int ppo_norm_set_stats(ppo_handle* h, int which, const float* mean, const float* var, double count);

/* ---- device-resident rollout: Runner::run (ppo2/runner.hpp:56-157) with buffers kept in HBM ---------------
 * Buffers are time-major [T,E,...]; the reference's env-major row r = e*T + t (runner.hpp:136-152) is mapped
 * at gather time, nothing is transposed. */
int ppo_rollout_alloc(ppo_handle* h, int32_t n_envs, int32_t n_steps);
/* host-Env path (an Env behind env/env.hpp steps on the host):
 *   reset   : EnvNormalize::reset + Runner ctor (runner.hpp:48-50): normalise raw obs, dones = 0
 *   act     : policy step on the current obs -> rollout[t]; actions copied back for Env::step (runner.hpp:75-116)
 *   observe : EnvNormalize::step on the raw step result; stores reward[t]; becomes the current obs/dones
 * Call pattern per rollout: act(0), observe(0), act(1), ... observe(T-1), finish.  With <= 64 environments on the narrow path
 * (the reference's setting is ONE) and no explicit noise, the library serves the whole rollout from one resident kernel: act /
 * observe then only exchange the actions and the transition through pinned memory.  That is invisible to the caller: any other
 * entry point called in between sees the state the step-by-step path would show (the kernel is retired and relaunched as
 * needed), values[t] are available after ppo_rollout_finish, and a host that pauses only costs the kernel a bounded wait. */
int ppo_rollout_reset(ppo_handle* h, const float* raw_obs);
int ppo_rollout_act(ppo_handle* h, int32_t t, const float* noise, float* actions_out);
/* ppo_rollout_act under an action mask [E, A] (needs ppo_set_action_masking on): the mask is stored in row t of the rollout's mask buffer and the step samples
 * under it.  mask == NULL, and plain ppo_rollout_act on a masking handle, mean an all-ones row (the unmasked kernel; the row is recorded as ones). */
int ppo_rollout_act_masked(ppo_handle* h, int32_t t, const float* noise, const float* mask, float* actions_out);
/* One launch per env step for a NARROW DISCRETE handle behind a host Env (default off; opt-in per handle).  It takes effect on a categorical or multi-categorical
 * handle on which PPO_ACT_SHAPE_KERNELS took effect, without a communicator, with at most 32 environments, at most 64 observations and logits, the image + one row
 * group within 160 KB of LDS, and PPO_HIP_NO_HOST_FUSED unset.  Then ppo_rollout_act[_masked] runs narrow_host_step_kernel<cat|mcat[,mask]>: ONE launch reads the
 * last transition from the handle's pinned block, books EnvNormalize::step for it, normalises, runs the policy tower, samples with narrow_step_kernel<cat|mcat[,mask]>'s
 * head arithmetic (same uniforms for the same seed or explicit noise), stores the [E, 1 | K] actions into pinned memory and raises a completion word; the mask of
 * ppo_rollout_act_masked is copied into a pinned [E, A] block that the kernel reads in place and stores into row t of the mask buffer (the plain call on a masking
 * handle: the unmasked form, a row of ones).  ppo_rollout_observe only posts the transition; values[t] are computed by one batched pass at ppo_rollout_finish.
 * With or without explicit noise; never a resident form.  ppo_kernel_counts names, one per act launch, counted INSTEAD of the act launches of
 * "narrow_step_kernel<cat|mcat[,mask]>": "narrow_host_step<cat>", "narrow_host_step<cat,mask>", "narrow_host_step<mcat>", "narrow_host_step<mcat,mask>".
 * Anywhere else -- a Gaussian handle (its own fused and resident forms are not affected), a discrete handle that is not on the narrow family, more than 32
 * environments, data parallel -- the call is accepted and nothing changes: same bits, same ppo_kernel_counts.  Against the per-step form of the same handle the
 * normalised observations differ by rounding (the fused step scales with the variance in place of the per-step form's standard deviation pass), as the Gaussian
 * fused form does against its general path; with normalisation off the two forms give the same bits.  Measured per env step: DESIGN.md section 5. */
int ppo_set_host_step_fused(ppo_handle* h, int32_t on);   /* before ppo_rollout_alloc; changing it drops an allocated rollout, like ppo_set_action_masking */
int ppo_host_step_fused(const ppo_handle* h);             /* the setting (0 / 1), not whether it took effect: ppo_kernel_counts says that */
/* The RESIDENT rollout for a NARROW DISCRETE handle: one launch per rollout (default off; opt-in per handle).  It takes effect on a categorical or multi-categorical
 * handle on which PPO_ACT_SHAPE_KERNELS took effect, without a communicator, with at most 64 environments, at most 64 observations and logits, and the image + the
 * rollout state of the handle's environments within 160 KB of LDS.
 *   Device env (ppo_collect_synthetic), unless PPO_HIP_NO_PERSISTENT_COLLECT=1: ONE launch of narrow_rollout_kernel<cat|mcat> runs all T env steps, with or without
 * explicit [T, E, A] uniforms; the values come from one batched pass afterwards.  Every field has the bits of the per-step form.  A masking handle samples
 * unmasked and records ones, as before.
 *   Host Env (ppo_rollout_act[_masked]), when no explicit noise is passed and PPO_HIP_NO_HOST_RESIDENT / PPO_HIP_NO_HOST_FUSED are unset: the kernel stays on the GPU
 * for the whole rollout, as the Gaussian resident form does (above): actions and transitions travel through pinned memory behind sequence words, every device-side
 * wait is bounded (PPO_HIP_HOST_POLLS), a kernel that gave up waiting parks itself and is relaunched by the next act, and any other entry point called in between
 * sees the state the per-step form would show.  With explicit noise the step leaves the resident form: the fused step if ppo_set_host_step_fused is also on and took
 * effect, the per-step form otherwise.  With both settings on and no explicit noise the resident form serves the step.
 *   The mask protocol: ppo_rollout_observe(t - 1) lets the running kernel start row t at once, but the mask of row t is known only at ppo_rollout_act_masked(t, ..).
 * A masking handle therefore runs the <..,mask> instantiation for plain and masked steps alike: the call copies the checked mask (the plain call: ones) into a
 * pinned [E, A] block and raises a third sequence word; the kernel runs row t's policy tower without waiting, waits (bounded) for that word before it samples, reads
 * the block in place and stores it into row t of the mask buffer as the host wrote it.  A refused mask launches nothing and posts nothing; the rollout goes on with
 * the next valid call.
 *   ppo_kernel_counts names, one per launch (a rollout behind a host Env: one, plus one per relaunch of a parked kernel), counted INSTEAD of the act launches of
 * "narrow_step_kernel<cat|mcat[,mask]>" / "narrow_host_step<..>": "narrow_rollout<cat>", "narrow_rollout<cat,mask>", "narrow_rollout<mcat>",
 * "narrow_rollout<mcat,mask>".  Anywhere else -- a Gaussian handle (its own resident forms are not affected), a discrete handle that is not on the narrow family,
 * more than 64 environments, a state too large for LDS, data parallel -- the call is accepted and nothing changes: same bits, same ppo_kernel_counts.
 * On the device env every field and both statistics have the bits of the per-step launches, with normalisation on or off (the kernel sums a batch's moments in
 * the order of the per-step form's statistics kernel); behind a host Env the same holds with normalisation off, and with it on the two forms are held to the
 * project's tolerances.
 * Measured per env step ((18, 6, [64,64]), resident against per-step): behind a host Env 17.6 against 34.7 us at one environment (masked 21.0
 * against 38.8; (6, 6, 6) masked 23.6 against 40.1), 22.1 against 36.8 at 32, 27.5 against 34.1 at 64 ((6, 6, 6) masked 36.5 against 40.5); on the device env 6.7
 * against 25.1 us of GPU time at one environment, 12.8 against 26.3 at 64. */
int ppo_set_rollout_resident(ppo_handle* h, int32_t on);   /* before ppo_rollout_alloc; changing it drops an allocated rollout, like ppo_set_host_step_fused */
int ppo_rollout_resident(const ppo_handle* h);             /* the setting (0 / 1), not whether it took effect: ppo_kernel_counts says that */
int ppo_rollout_observe(ppo_handle* h, int32_t t, const float* raw_obs, const float* raw_rew, const float* dones);
/* Time-limit truncations (no reference counterpart).  The `done` of step t of the environments env_ids [count] (int32) was raised by a time limit, not by a
 * terminal state; terminal_raw_obs [count, O] are the RAW observations those episodes ended on (raw_obs of ppo_rollout_observe holds the observation after the
 * reset).  Call it after ppo_rollout_observe(h, t, ..) and before the next ppo_rollout_act / ppo_rollout_finish, any number of times.  It only appends to a
 * host-side list of the handle: nothing is enqueued, and it does not depend on which rollout form serves the handle (a resident kernel keeps running).
 * ppo_rollout_finish then bootstraps those rows: the terminal observations are scaled and clipped with the observation statistics AS THEY STAND AT THE FINISH
 * (after the last transition is booked -- exactly like the end-of-rollout bootstrap observation; they never update obs_rms; with norm_obs == 0 they pass through),
 * valued in one batched pass with the weights the rollout was collected with, and GAE runs in ppo_gae_ex's form.  The stored rewards (after EnvNormalize's
 * scaling and clip) are the ones that get gamma * V added; the reward normaliser's return accumulator and ret_rms are not touched.  Data parallel: every rank
 * marks and bootstraps its own rows.
 * Errors, each leaving the list as it was: no rollout allocated, t out of range or not the step of the last ppo_rollout_observe, an env id out of range or named
 * twice, (t, env) already marked, an env whose done in step t is 0, count < 0.  count == 0 is a no-op.  The list is emptied by ppo_rollout_finish (after use),
 * ppo_rollout_reset and ppo_rollout_alloc.  A rollout without marks enqueues exactly the launches it enqueued before this entry point existed. */
int ppo_rollout_mark_truncated(ppo_handle* h, int32_t t, int32_t count, const int32_t* env_ids, const float* terminal_raw_obs);
/* bootstrap value + GAE (runner.hpp:134, 159-191); with marked truncations: their value pass, the scatter into the [T,E] table (tval_scatter_kernel) and the
 * truncation form of GAE (ppo_kernel_counts: "gae_kernel<trunc>" / "gae_long_kernel<trunc>") */
int ppo_rollout_finish(ppo_handle* h, float gamma, float lam);
/* device-env path: the whole T-step collect against the on-device seeded synthetic env (obs ~ U(-1,1)^O,
 * reward ~ U(-1,1), done ~ Bernoulli(1/300), keyed by (seed, global env id, step counter)); env ids start at
 * env0 (rank sharding).  first != 0 performs the reset (step counter step0), otherwise continues from the carried
 * obs/dones.  noise [T,E,A] or NULL.  Ends with bootstrap + GAE.
 * Categorical handle: noise [T,E,A] (ppo_collect_synthetic) / [E,A] (ppo_rollout_act) are uniforms, actions_out of ppo_rollout_act is [E]. */
/* Every done of the seeded device env is a terminal state: it has no terminal observation, ppo_rollout_mark_truncated does not apply to this path. */
/* The seeded device env has no notion of legality either: on a masking handle ppo_collect_synthetic samples unmasked and records every row's mask as ones. */
int ppo_collect_synthetic(ppo_handle* h, uint32_t seed, int32_t env0, uint32_t step0, int first,
                          const float* noise, float gamma, float lam);
/* field: 0 obs[T,E,O] 1 actions[T,E,A] 2 values 3 neglogp 4 dones 5 rewards 6 returns (all [T,E]); a categorical handle's field 1 is [T,E], a multi-categorical one's [T,E,K].
 * 7 (download only; an upload is refused): terminal values [T,E] as the last ppo_rollout_finish used them -- V(terminal observation) on the marked rows, 0 elsewhere,
 * all zeros when that finish had no marks.
 * 8: action masks [T,E,A] of a masking handle (refused with masking off; an uploaded row without an allowed category is refused). */
int ppo_rollout_download(ppo_handle* h, int field, float* dst, int64_t count);
int ppo_rollout_upload(ppo_handle* h, int field, const float* src, int64_t count);

/* ---- the whole minibatch-update phase of PPO2::learn (ppo2/ppo2.hpp:274-335) on the resident rollout ------
 * perms [noptepochs, B] int32: perms[ep][i] = destination row of flattened source row i in epoch ep
 * (out.row(perm[i]) = in.row(i), ppo2.hpp:291-296), or NULL = fresh on-device pseudo-random permutation per
 * epoch keyed by (seed, epoch).  loss_rows [noptepochs*nminibatches, 5] (may be NULL); mean_losses = their
 * column means (ppo2.hpp:335).  One HIP launch sequence per minibatch, replayed from a hipGraph (the reference's own shape -- [64,64], minibatches of <= 64 rows --
 * runs all minibatches of an epoch inside ONE resident launch; same results bit for bit, PPO_HIP_NO_NARROW_EPOCH=1 keeps the launches). */
int ppo_update(ppo_handle* h, float lr, float cliprange, int32_t noptepochs, int32_t nminibatches,
               const int32_t* perms, uint64_t seed, float* loss_rows, float mean_losses[5]);

/* ---- data parallel: one process per GPU, RCCL over xGMI (new work; the reference has no collectives) -------
 * uid = 128-byte ncclUniqueId made by rank 0 (ppo_dist_unique_id) and broadcast by the launcher.  After init,
 * ppo_train_step / ppo_update all-reduce (sum) the flat gradient + loss sums across ranks between the backward
 * and the clip+Adam launches, and ppo_norm_* merge their batch moments across ranks. */
int ppo_dist_unique_id(char uid[128]);
/* (a categorical handle created with PPO_ACT_SHAPE_KERNELS is refused: "... data parallel is not supported for a categorical handle created with PPO_ACT_SHAPE_KERNELS";
 *  a multi-categorical one on which that flag took effect (ppo_create_multi_ex) likewise: "... for a multi-categorical handle created with PPO_ACT_SHAPE_KERNELS";
 *  one on which PPO_ACT_PAIR_KERNELS took effect likewise: "... data parallel is not supported for a categorical handle created with PPO_ACT_PAIR_KERNELS";
 *  a multi-categorical one on which PPO_ACT_PAIR_KERNELS took effect: "... data parallel is not supported for a multi-categorical handle created with PPO_ACT_PAIR_KERNELS";
 *  a multi-binary one on which PPO_ACT_BINARY_SHAPE_KERNELS took effect: "... data parallel is not supported for a multi-binary handle created with PPO_ACT_BINARY_SHAPE_KERNELS";
 *  a multi-binary one on which PPO_ACT_BINARY_PAIR_KERNELS took effect: "... data parallel is not supported for a multi-binary handle created with PPO_ACT_BINARY_PAIR_KERNELS";
 *  a categorical PPO_BF16 handle (PPO_ACT_BF16_HEAD) likewise: "... data parallel is not supported for a categorical PPO_BF16 handle created with PPO_ACT_BF16_HEAD";
 *  a multi-categorical PPO_BF16 handle (PPO_ACT_BF16_MULTI_HEAD): "... data parallel is not supported for a multi-categorical PPO_BF16 handle created with PPO_ACT_BF16_MULTI_HEAD") */
int ppo_dist_init(ppo_handle* h, int32_t world_size, int32_t rank, const char uid[128]);
int ppo_dist_world(const ppo_handle* h);
/* What a reader of a scaling run needs in order to check the ranks (all out-pointers optional): the number of ranks the
 * COMMUNICATOR reports (ncclCommCount; -1 when the library has no such entry point, 0 without a communicator), this handle's HIP
 * device ordinal, its PCI bus id ("0000:05:00.0") and the path of the collective library that was actually loaded. */
int ppo_dist_info(ppo_handle* h, int32_t* comm_nranks, int32_t* device, char pci_bus_id[32], char library[256]);
/* 1 when ppo_update replays the collectives from its hipGraph (the communicator's library passed the capture probe of
 * ppo_dist_init, or PPO_HIP_GRAPH_RCCL=1), 0 when they are issued eagerly between the launches */
int ppo_dist_graph_collectives(const ppo_handle* h);
/* One-shot all-reduce over peer-mapped buffers (xGMI is point-to-point: every rank pushes its vector into its slot of every
 * peer's gather region, raises a flag there, and sums the slots of its own region in rank order -- one hop instead of a
 * ring's 2(W-1), same summation order on every rank).  One node, world_size <= 8.
 *   ppo_dist_peer_export: after ppo_dist_init; allocates this rank's gather region and returns its 64-byte IPC handle.
 *   ppo_dist_peer_attach: COLLECTIVE; handles = world_size x 64 bytes in rank order (all-gathered by the launcher).  Maps the
 *     peers' regions, runs a known-answer exchange and lets the ranks agree on the outcome over the communicator: every
 *     collective of ppo_update / ppo_rollout_* / ppo_norm_* whose payload fits then uses the peer kernels (plain launches,
 *     replayed from the update's hipGraph); if any rank fails to map a peer or fails the probe, all ranks stay on RCCL.
 *     PPO_HIP_PEER_REDUCE=0 keeps RCCL; PPO_HIP_PEER_TIMEOUT_MS bounds the wait on a peer's flag (default 10 s), after which
 *     the next ppo_update / ppo_rollout_finish / ppo_collect_synthetic returns an error instead of hanging the device.
 *     The call ends with a collective over the communicator, so no rank returns before every rank has finished its probe.
 *   ppo_dist_peer_active: 1 when the peer path is in use.   ppo_dist_peer_enable: switch between the two paths after a
 *     successful attach (collectively, at the same point on every rank).
 *   With the peer path on, a [256,256] handle pushes its gradient tiles from inside the weight-gradient kernel and adds the ranks up inside the Adam launch
 *     (no push / sum launches; PPO_HIP_NO_PEER_TILES=1 restores them).  Single-rank kernels whose workgroups wait for EACH OTHER while holding a CU (the bf16
 *     path's chained layers) are switched off when two ranks of the job share a device: ppo_dist_init compares the ranks' PCI ids over the communicator.
 *     The data-parallel forms that wait on the PEERS' flags (the tile push, adam_kernel's meeting) stay on there -- one device with several ranks is how this path
 *     is tested -- and every such wait is bounded (PPO_HIP_PEER_TIMEOUT_MS): a rank whose peers cannot become resident beside it reports an error, it does not hang. */
int ppo_dist_peer_export(ppo_handle* h, char handle[64]);
int ppo_dist_peer_attach(ppo_handle* h, const char* handles);
int ppo_dist_peer_active(const ppo_handle* h);
int ppo_dist_peer_enable(ppo_handle* h, int on);
/* Sampling under data parallelism.  Default (0): every rank shuffles its OWN B rows, global minibatch k = the union of the ranks'
 * local minibatches k (a stratified form of the reference's shuffle; nothing but gradients and statistics crosses ranks).
 * 1 = the reference's literal scheme (ppo2/ppo2.hpp:288-307): ONE permutation of the B * world rows of all ranks per
 * epoch -- the same explicit `perms` [epochs][B * world] on every rank, or the same `seed` -- after an all-gather of the rollout
 * rows (ncclAllGather, once per ppo_update); rank r trains rows [r M, (r + 1) M) of every global minibatch of M * world rows.
 * A row index is e_global * T + t with e_global = rank * n_envs + e (runner.hpp:136-152 over the environments of all ranks). */
int ppo_dist_global_shuffle(ppo_handle* h, int on);
/* bf16 path under a communicator of more than one rank (collective library, not the peer regions): the gradient of a train step leaves in BUCKETS -- last layer + heads
 * first -- each bucket's ncclAllReduce on a second stream under the remaining backward and weight-gradient launches (default on; 0 = one all-reduce of the whole vector behind
 * them; 2 = also under a one-rank communicator, for measuring what the per-layer launches cost a rank).  Collective: call it at the same point on every rank.
 * No reference counterpart (its job is one process); DESIGN.md section 6. */
int ppo_dist_bucketed(ppo_handle* h, int on);

/* ---- measurement hooks ----------------------------------------------------------------------------------
 * per-kernel device time (ms) accumulated with hipEvents on the handle's stream since the last reset;
 * names/values are parallel arrays; returns the number of timed kernel classes */
int ppo_prof_enable(ppo_handle* h, int on);
int ppo_prof_read(ppo_handle* h, int max, char names[][32], double* total_ms, int64_t* launches);
int ppo_sync(ppo_handle* h);
/* which kernel VARIANT the calls so far took: the library picks its kernels from the shape, and a caller or a
 * test can ask which ones were ENQUEUED since ppo_create (a hipGraph capture counts once, its replays do not).  names: e.g.
 * "train8_kernel", "train8_kernel<cat>", "train8_kernel<mcat>", "weight_grad_assemble_kernel", "narrow_train_kernel<static>", "narrow_train_kernel<cat>", "narrow_epoch_kernel", "narrow_rollout1_kernel"; returns the count of entries.
 * ppo_kernel_counts is FROZEN at its 60 rows: callers hold its row count fixed.  Variants added later ("narrow_step_kernel<mbin>", "narrow_train_kernel<mbin>") appear
 * only in ppo_kernel_counts_all: the 60 in the same order, then those two.  Buffers of 64 entries hold either.
 * ppo_kernel_counts_all is FROZEN in turn, at its 62 rows: a caller holds that row count fixed too, so no fixed-length list can take a new variant.  Variants added
 * after it ("train8_kernel<mbin>") are reached BY NAME: ppo_kernel_count returns the count of any variant of this build, the 62 included, or -1 where no variant has
 * that name; ppo_kernel_variant_name(i) enumerates the names, i = 0, 1, .. until it returns NULL.  That list GROWS between versions (at most 64 names of at most 31
 * characters): walk it to the NULL, never hold its length. */
int ppo_kernel_counts(ppo_handle* h, int max, char names[][32], int64_t* enqueued);
int ppo_kernel_counts_all(const ppo_handle* h, int32_t max, char (*names)[32], int64_t* counts);
int64_t     ppo_kernel_count(const ppo_handle* h, const char* name);  /* any variant by name, later ones included; -1: no variant has that name */
const char* ppo_kernel_variant_name(int32_t i);                        /* i-th variant of this build, NULL past the last: the list GROWS between versions */

/* ---- debug: a raw device buffer by name, padding included (the getters above copy the dense part of every tensor) ----------------
 * "theta" "adam_m" "adam_v" (padded), "thetaT" / "par" (the transposed and small-parameter mirrors the train kernels read), "grad" (+ its tail), "sumsq", "beta_pow", "hyper",
 * "norm_out", "dw2_parts", the last train step's workspaces ("x0g" "dmug" "h_pi_0" ... "slots_pi" "slabs"), the gathered epoch ("mb_obs" ... "gidx" "advstats" "keys"), the
 * narrow path's packed image and second weight set ("nw_img" "nw_theta1" ...), the normaliser's state.
 * A PPO_BF16 handle's workspaces (0 words on every other handle; "slots_pi" / "slots_vf", "slabs", "theta" and "grad" are shared with the fp32 path): "bf_theta" (bf16 operand
 * mirror of "theta", same padded offsets), "bf_x0" (staged observations, bf16 [Rcap][Kp0]), "bf_h_pi_<l>" / "bf_h_vf_<l>" (tanh outputs of hidden layer l = 0 .. PPO_MAX_LAYERS - 1,
 * bf16 [Rcap][Hp_l]), "bf_dy_pi_<l>" / "bf_dy_vf_<l>" (gradients w.r.t. the pre-activations, same shape), "bf_head_pi" / "bf_head_vf" (fp32 [4][Rcap][Ap]: the head GEMM's partial
 * products per reduction range, bias in range 0; the value is column 0), "bf_dhead_pi" / "bf_dhead_vf" (bf16 [Rcap][Ap]: loss gradient w.r.t. the head outputs) and "bf_dbias" (fp32
 * [row tiles][sum of Hp_l over towers and layers]: per-row-tile bias-gradient sums; tower-major, then layer).  Rcap = the largest row count seen so far rounded up to 128; a bf16
 * buffer of N elements reads as N / 2 words (view the words as uint16 for the bit patterns).  tests/test_bf16_stages.py checks every stage of the path through them.
 * *count = the buffer's length in 4-byte words (0: not used by this shape);
 * at most max_count words are copied.  Two runs that must agree bit for bit are compared buffer by buffer with it (tests/test_other_shapes.py).  No reference counterpart. */
int ppo_debug_buffer(ppo_handle* h, const char* name, float* dst, int64_t max_count, int64_t* count);
/* debug: leave `word` in every LDS word of every CU (a launch of whole-CU workgroups on the handle's stream, synchronised).  A kernel that reads LDS it never wrote sees
 * what the previous workgroup on its CU left there; with a NaN pattern in place such a read shows in the results (tests/test_race_guards.py).  No reference counterpart. */
int ppo_debug_poison_lds(ppo_handle* h, uint32_t word);
/* debug: the node types of the hipGraph the last ppo_update captured: counts = {kernel, memset, memcpy, other}; -1 when the handle holds no graph.  The library's rule is
 * kernel nodes only (a memset node replayed out of order on ROCm 7.0.2: DESIGN.md section 9). */
int ppo_debug_graph_nodes(ppo_handle* h, int32_t counts[4]);
/* debug: raise the error word of the bf16 path's chained launch as a failed hand-off would; the next call that chains its layers must report it (ppo_step / ppo_value /
 * ppo_act_deterministic repeat their pass layer by layer; the rollout calls and ppo_update return the error) and the handle launches layer by layer from then on. */
int ppo_debug_raise_chain_error(ppo_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* PPO_HIP_H */
