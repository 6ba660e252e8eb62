// ppo_train8.hpp -- train model forward + loss + backward of one 16-row tile, 8 waves per workgroup, for hidden [256,256] with any
// observation / action width up to 64 (BASELINE configs[2] is 18 / 18; the reference's other hexapod shape is 36 / 18,
// env/hexapod_closed_loop_env.hpp:20).  Same arithmetic, slots and workspaces as train_fwd_bwd_kernel (G:6889-23699 minus the weight
// gradients); what changes is who does what inside the workgroup:
//   * M = 2048 rows give exactly one row tile per CU and tower, so the only latency hiding available is a second wave per SIMD:
//     the two 256 x 256 products (second layer forward, its transpose backward) are split over K between wave w and wave w + 4
//     (same SIMD, same 64 output columns, k in [0,128) / [128,256)): one wave's weight stream, LDS reads and waits are covered by
//     the other's matrix instructions.  The two halves meet in LDS: each wave hands the other the 8 accumulator values it does
//     not finish, and finishes (bias + tanh / TanhGrad, LDS + workspace stores) the other 8 -- rows {0,1} / {2,3} of every
//     4-row group, so that the workspace stores stay 16 bytes per lane;
//   * the three thin products (first layer, policy head transposed; the policy head itself is an 8-way K split) give every
//     wave 32 output columns: half the epilogue per wave;
//   * the loss phase has one lane per (row, action) (two actions per lane when the action tile is 64 wide) instead of two serial
//     passes over 16 lanes per row.
// The padded widths of the observation and action tiles (KP0, AP: 32 or 64) are template parameters -- every loop is compile-time;
// the dense widths O and A are uniform run-time values.  The first layer's weights and the first ring stage of the second layer are
// requested at kernel entry behind the input loads, the second stage behind the prologue's barrier (T8_PRO), the policy head's weights and their transpose behind
// the second layer's product (T8_HEADW) (one workgroup of 8 waves per CU: 256 registers per wave).
#pragma once
#include "ppo_kernels.hpp"

#define T8_THREADS 512
#define T8_LD 260                 // 256 + LDS_PAD
// LDS carve (floats) for an observation tile of KP0 and an action tile of AP columns
template <int KP0, int AP>
struct T8L {
    static constexpr int LD0 = KP0 + LDS_PAD, LDM = AP + LDS_PAD;
    static constexpr int NPAR = 3 * 256 + 2 * AP + 4;                      // biases (2 x 256) | b_mu | logstd | w_v | b_v (NetDev::par_*)
    static constexpr int X0 = 0, H1 = X0 + 16 * LD0, H2 = H1 + 16 * T8_LD, D2 = H2 + 16 * T8_LD, D1 = D2 + 16 * T8_LD,
                         MU = D1 + 16 * T8_LD, PAR = MU + 16 * LDM, ACT = PAR + NPAR + 4, DLS = ACT + 16 * AP, ROWV = DLS + 16 * AP,
                         MISC = ROWV + 32, TOTAL = MISC + 128;
    // the <.., MULTI> instantiations only: a row's K action indices, [16][PPO_MAX_COMPONENTS_DEV], behind the carve every other instantiation keeps
    static constexpr int MACT = TOTAL, TOTAL_M = MACT + 16 * PPO_MAX_COMPONENTS_DEV;
};

#ifndef T8_PRO
#define T8_PRO 1                  // where the second layer's first two ring stages are requested: 0 both in the prologue, 1 the second one behind the prologue's
                                  // barrier (it lands while the first layer runs; the prologue's request burst is 32 KB per wave shorter: 41.7 -> 40.6 us per
                                  // train step), 2 both behind the barrier (42.6 us: the first layer's end then waits for them)
#endif
#ifndef T8_W1T
#define T8_W1T 0                  // where the backward product's first two W1^T stages are requested: 0 before the K-halves' exchange, 1 after it, 2 one after it + one behind the epilogue's barrier
#endif
#ifndef T8_HEADW
#define T8_HEADW 2                // where the policy tower requests its head's weights (W_mu rows and W_mu^T: 8 KB per wave, first read behind the second layer): 0 in the
                                  // prologue's burst (39.04 / 38.93 / 39.07 us per train step), 1 behind the prologue's barrier, behind the second ring stage (40.12 /
                                  // 40.06 / 39.95: the 16 requests per wave cost the first layer what they saved the prologue, and more), 2 behind the second layer's
                                  // product, in front of the W1^T stages (38.76 / 38.60 / 38.68: the one stretch where the memory pipe is idle; in-order return puts them
                                  // in front of stages nobody reads for 12 k cycles).  W_mu rows at 1 and W_mu^T at 2: 41.17 / 41.34 / 40.93, not kept in the source.
#endif
#ifndef T8_WT
#define T8_WT 1                   // workspace stores write-through (sc1): drain while the kernel computes instead of at its end
#endif
__device__ __forceinline__ void t8_st_wt2(float* p, float x, float y) {
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t v = {x, y};
    if constexpr (T8_WT != 0) asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(v) : "memory");
    else *reinterpret_cast<float2*>(p) = make_float2(x, y);
}
// sum over the 32 lanes of a half-wave
__device__ __forceinline__ float t8_sum32(float v) { v = group16_sum(v); v += __shfl_xor(v, 16); return v; }
// maximum over the same 32 lanes, the same butterfly (the categorical head's row maximum; -inf marks a lane without an allowed category)
__device__ __forceinline__ float t8_max32(float v) {
    v = tf_max(v, dpp_move<0xB1>(v)); v = tf_max(v, dpp_move<0x4E>(v)); v = tf_max(v, dpp_move<0x141>(v)); v = tf_max(v, dpp_move<0x140>(v));
    return tf_max(v, __shfl_xor(v, 16));
}

// one 32-deep stage of a [16 x 64] output chunk: 8 k-steps x 4 column tiles
__device__ __forceinline__ void t8_mma_stage(const WFrag<4, 2>& f, f32x4 (&acc)[4]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const float av[4] = {f.a[q].x, f.a[q].y, f.a[q].z, f.a[q].w};
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], f.v[4 * q + s][j], acc[j], 0, 0, 0);
    }
}
// a (16 KS)-deep product into 16 CT output columns per wave (CT interleaved column tiles)
template <int CT, int KS>
__device__ __forceinline__ void t8_mma_small(const WFrag<CT, KS>& f, const float* Xs, int ldx, int c, int g, f32x4 (&acc)[CT]) {
#pragma unroll
    for (int q = 0; q < KS; ++q) {
        const float4 a4 = *reinterpret_cast<const float4*>(Xs + c * ldx + 16 * q + 4 * g);
        const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < CT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], f.v[4 * q + s][j], acc[j], 0, 0, 0);
    }
}

// The K-split 256 x 256 product of wave (p = column block, kh = K half): Y[16, 64p..64p+63] partial over k in [128 kh, 128 kh + 128).
// fr[0], fr[1] hold the first two stages (requested by the caller); returns the partial accumulators.  `rot` (wave-uniform, 0..3)
// rotates the order in which the four 32-deep stages are taken: the 32 workgroups of an XCD stream the SAME weights, and in
// lockstep they would all ask one 32 KB block of L2 at a time; rotated by row tile they spread over the whole matrix.
#ifndef T8_ROTATE
#define T8_ROTATE 0                // measured: 42.0 us per train step rotated against 41.2 (no L2 hot spot to avoid; dynamic stage addresses cost)
#endif
__device__ __forceinline__ int t8_stage_row(int st, int rot) { return T8_ROTATE ? 32 * ((st + rot) & 3) : 32 * st; }
__device__ __forceinline__ void t8_big_product(WFrag<4, 2> (&fr)[3], const float* Wk /* W + 128 kh rows */, const WOff<2>& off, const float* Xs /* tile + 128 kh */,
                                               int c, int g, int rot, f32x4 (&acc)[4]) {
    auto load_a = [&](WFrag<4, 2>& f, int st) __attribute__((always_inline)) {
        const int k0 = t8_stage_row(st, rot);
#pragma unroll
        for (int q = 0; q < 2; ++q) f.a[q] = *reinterpret_cast<const float4*>(Xs + c * T8_LD + k0 + 16 * q + 4 * g);
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    load_a(fr[0], 0); load_a(fr[1], 1);
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        __builtin_amdgcn_sched_barrier(0);
#ifdef T8_NOLOAD
        if (st + 2 < 4) load_a(fr[(st + 2) % 3], st + 2);      // timing experiment only: results are wrong
#else
        if (st + 2 < 4) { load_a(fr[(st + 2) % 3], st + 2); load_w_stage<4, 2>(fr[(st + 2) % 3], Wk + (size_t)t8_stage_row(st + 2, rot) * 256, off); }
#endif
        t8_mma_stage(fr[st % 3], acc);
#ifndef T8_NOSCHED
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
        for (int t = 0; t < 8; ++t) { __builtin_amdgcn_sched_group_barrier(0x008, 4, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); }
#endif
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the two K halves meet: wave kh hands rows {2,3} (kh = 0) / {0,1} (kh = 1) of every 4-row group to its partner and returns the
// finished values of the rows it keeps: out[j][i] = row 4g + 2 kh + i, column 64 p + 4 c + j  (kh0 + kh1 in that order on both sides)
__device__ __forceinline__ void t8_exchange(const f32x4 (&acc)[4], float* xch, int p, int kh, int lane, float (&out)[4][2]) {
    float* mine = xch + ((p * 2 + kh) * 64 + lane) * 8;
    const float* theirs = xch + ((p * 2 + (kh ^ 1)) * 64 + lane) * 8;
    const int give = kh ? 0 : 2;                    // first of the two rows handed over
    *reinterpret_cast<float4*>(mine) = make_float4(acc[0][give], acc[1][give], acc[2][give], acc[3][give]);
    *reinterpret_cast<float4*>(mine + 4) = make_float4(acc[0][give + 1], acc[1][give + 1], acc[2][give + 1], acc[3][give + 1]);
    lds_barrier();
    const float4 t0 = *reinterpret_cast<const float4*>(theirs), t1 = *reinterpret_cast<const float4*>(theirs + 4);
    const float th[2][4] = {{t0.x, t0.y, t0.z, t0.w}, {t1.x, t1.y, t1.z, t1.w}};
    const int keep = kh ? 2 : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) out[j][i] = kh ? th[i][j] + acc[j][keep + i] : acc[j][keep + i] + th[i][j];
}

// The kernel's body.  The big workspaces leave write-through (T8_WT: they drain while the kernel computes); the small outputs -- x0g, dmug, slots -- are plain
// stores left to the kernel boundary.  (Round 5 also called this body as the first phase of a fused train + weight-gradient launch; measured slower twice and removed
// in round 6: profiles/r05_a_*, branch experiments-r05.)  bx / by / gx: the launch's block index (x, y) and grid width.
// CAT: categorical head (a handle created with PPO_ACT_CATEGORICAL | PPO_ACT_PAIR_KERNELS) -- train_fwd_bwd_kernel<.., CAT>'s arithmetic in this kernel's geometry.
// `actions` holds ONE float per row, the category index: the prologue parks it in MISC[64 + row] (the loss terms use MISC[0, 64)).  The logits are mu[q]; lane ej of a
// row owns categories ej and, with a 64-column tile, ej + 32; maximum, normaliser, the action's logit and the entropy meet over the row's 32 lanes.  d logits go where
// d mu goes (the MU tile, dmug); the DLS tile and the slot_aux words are zeros (no pi/logstd).  Only the prologue's action load and the head block differ.
// MASK (with CAT): thread (er, ej) requests a.mask[(row0 + er) nA + ej + 32 q] where the Gaussian form requests its action elements and parks them in the ACT tile; the
// same lane reads them back.  Forbidden categories are excluded from maximum, normaliser, neglogp and entropy and their d logits are exactly +0; a dead row reads nothing
// and counts every category as allowed.  A row of ones gives the unmasked form's bits.  Nothing is indexed with the action or the mask.
// MULTI (with CAT): K categorical components over the one logits row (TrainArgsM::comp), train_fwd_bwd_kernel<.., MULTI>'s arithmetic in this kernel's geometry.
// `actions` holds K floats per row: threads 0..255 request element (row tid >> 4, component tid & 15) with the other inputs and park it in the MACT region (the
// MISC words hold one index per row; the ACT tile is the mask's).  Two wave-uniform walks over the components, every lane taking part in every reduction with -inf / 0
// for the elements outside the component: the first leaves each element its own component's maximum, so a0 and exp are formed ONCE per element; the second forms
// the component's normaliser, action a0 and entropy, adds neglogp and entropy up in component order and leaves each element its own component's z, log z, H and
// action column for the gradient.  A lane's two elements may belong to two components (or both to one that spans column 32): every select is per element.
// One component is the <cat> form statement by statement.  No barrier beyond the <cat> form's; nothing is indexed with an action or a mask value.
// BIN (without CAT): multi-binary head (a handle created with PPO_ACT_MULTI_BINARY | PPO_ACT_BINARY_PAIR_KERNELS) -- train_fwd_bwd_kernel<.., MbinHead>'s arithmetic in
// this kernel's geometry.  `actions` holds A floats per row, each 0 or 1: the Gaussian form's prologue requests and parks them in the ACT tile unchanged, and the same
// lane reads them back.  The logits are mu[q]; the head is elementwise in the Gaussian branch's lane geometry: bern_parts is formed ONCE per element and serves
// neglogp, entropy and gradient; the row's neglogp and entropy are two t8_sum32 (padding columns add exactly 0).  d logits go where d mu goes; the DLS tile and the
// slot_aux words are zeros and par_ls is not read, as in the <cat> form.  No reduction, barrier or LDS region beyond the Gaussian form's.
template <int KP0, int AP, bool CAT = false, bool MASK = false, bool MULTI = false, bool BIN = false>
__device__ __forceinline__ void train8_body(const NetDev& net, const std::conditional_t<MULTI, TrainArgsM, TrainArgs>& a, float* lds, const unsigned bx, const unsigned by, const unsigned gx) {
    static_assert(CAT || !MASK, "action masks belong to the categorical head");
    static_assert(CAT || !MULTI, "the multi-categorical head is a form of the categorical one");
    static_assert(!(CAT && BIN), "the multi-binary head is a head of its own");
    typedef T8L<KP0, AP> L8;
    constexpr int KS0 = KP0 / 16, KSA = AP / 16;       // k-steps of 16 in the first layer / in the head's backward product
    constexpr int CTA = AP / 16;                       // column tiles of the policy head (all AP columns in every wave)
    constexpr int NX = KP0 / 32, NA = AP / 32;         // observation / action tile elements per thread ([16][KP0] and [16][AP] over 512 threads)
    int tower = (int)by;
    int rb = (gx % 8 == 0) ? (int)((bx % 8) * (gx / 8) + bx / 8) : (int)bx;
    if (a.xcd_map == 1 && gx % 4 == 0) {      // see train_fwd_bwd_kernel: XCD x = tower x & 1, row tiles of split x >> 1
        const int lid = (int)(bx + gx * by), x = lid & 7, q = lid >> 3;
        tower = x & 1;
        rb = (x >> 1) * (int)(gx / 4) + q;
    }
    tower = uni(tower); rb = uni(rb);
    const int row0 = rb * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = uni(tid >> 6);
    const int g = lane >> 4, c = lane & 15;
    const int p = wave & 3, kh = wave >> 2;
    const int rot = uni(rb & 3);
    const int nO = uni(net.O), nA = uni(net.A);
    float* slot = a.slots[tower] + (size_t)rb * net.slot_w;
    float* par = lds + L8::PAR;
    STAMP(0);
#ifdef PPO_STAMPS
    { const float probe = a.hyper[0]; asm volatile("" :: "v"(probe)); }      // (diagnostic builds: the kernarg round trip ends here)
    STAMP(20);
#endif
    // ---- prologue: every input load, then the weights the thin products need and the first two ring stages -------------------------
    const float* par_src = a.par + tower * net.par_total;
    float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < L8::NPAR / 4) pv = reinterpret_cast<const float4*>(par_src)[tid];         // biases | b_mu | logstd | w_v | b_v
    const int er = tid >> 5, ej = tid & 31;                                             // this thread's element(s) of a [16][32 q + ej] tile
    const bool erow_live = row0 + er < a.n;
    float ov[NX], av_[NA];
#pragma unroll
    for (int q = 0; q < NX; ++q) { ov[q] = 0.f; if (erow_live && ej + 32 * q < nO) ov[q] = a.obs[(size_t)(row0 + er) * nO + ej + 32 * q]; }
#pragma unroll
    for (int q = 0; q < NA; ++q) {
        av_[q] = 0.f;
        if constexpr (MASK) { if (tower == 0 && erow_live && ej + 32 * q < nA) av_[q] = a.mask[(size_t)(row0 + er) * nA + ej + 32 * q]; }
        else if constexpr (!CAT) { if (tower == 0 && erow_live && ej + 32 * q < nA) av_[q] = a.actions[(size_t)(row0 + er) * nA + ej + 32 * q]; }
    }
    float r0 = 0.f, r1 = 0.f, r2 = 0.f, s0 = 0.f, s1 = 1.f, rc = 0.f;
    float mk = 0.f;                                                                     // MULTI: action index of (row tid >> 4, component tid & 15)
    if constexpr (MULTI) {
        if (tower == 0 && tid < 16 * PPO_MAX_COMPONENTS_DEV && row0 + (tid >> 4) < a.n && (tid & 15) < a.comp.K) mk = a.actions[(size_t)(row0 + (tid >> 4)) * a.comp.K + (tid & 15)];
    }
    const bool explicit_adv = a.advs != nullptr;
    if (tid < 16 && row0 + tid < a.n) {
        const int src = row0 + tid;
        if (tower == 0) {
            r0 = explicit_adv ? a.advs[src] : a.returns[src]; r2 = a.old_neglogp[src];
            if (!explicit_adv) { r1 = a.old_values[src]; s0 = a.adv_stats[0]; s1 = a.adv_stats[1]; }
            if constexpr (CAT && !MULTI) rc = a.actions[src];                            // the row's category index
        } else { r0 = a.returns[src]; r2 = a.old_values[src]; }
    }
    const float* W0 = uni(a.theta + net.w_off[tower][0]);
    const float* W1 = uni(a.theta + net.w_off[tower][1]) + (size_t)(128 * kh) * 256;
    const float* W1T = uni(a.thetaT + net.wT_off[tower][1]) + (size_t)(128 * kh) * 256;
    const WOff<2> off_big = make_woff<2>(256, g, 64 * p + 4 * c);
    WFrag<2, KS0> wl0;
    WFrag<CTA, 2> whd;
    WFrag<2, KSA> whT;
    WFrag<4, 2> fr[3];
    load_w_stage<2, KS0>(wl0, W0, make_woff<KS0>(256, g, 32 * wave + 2 * c));
#if T8_PRO < 2
    load_w_stage<4, 2>(fr[0], W1 + (size_t)t8_stage_row(0, rot) * 256, off_big);
#endif
#if T8_PRO == 0
    load_w_stage<4, 2>(fr[1], W1 + (size_t)t8_stage_row(1, rot) * 256, off_big);
#endif
    // the policy head's weights and their transpose (T8_HEADW: where they are requested).  A macro, not a lambda: this kernel's time moves by 1.5 us per train step
    // with wrappers that change no instruction's meaning (profiles/EXPERIMENTS.md), so every placement keeps the statements themselves
#define T8_REQUEST_WHD() load_w_stage<CTA, 2>(whd, uni(a.theta + net.wmu_off) + (size_t)(32 * wave) * AP, make_woff<2>(AP, g, CTA * c))   /* rows 32w .. 32w+31 of W_mu [256][AP] */
#define T8_REQUEST_WHT() load_w_stage<2, KSA>(whT, uni(a.thetaT + net.wmuT_off), make_woff<KSA>(256, g, 32 * wave + 2 * c))               /* W_mu^T [AP][256] */
#if T8_HEADW == 0
    if (tower == 0) {
        T8_REQUEST_WHD();
        T8_REQUEST_WHT();
    }
#endif
    STAMP(21);
    // consume the inputs
    if (tid < L8::NPAR / 4) *reinterpret_cast<float4*>(par + 4 * tid) = pv;
#pragma unroll
    for (int q = 0; q < NX; ++q) {
        lds[L8::X0 + er * L8::LD0 + ej + 32 * q] = ov[q];
        if (tower == 0) st_wt<false>(a.x0g + (size_t)(row0 + er) * KP0 + ej + 32 * q, ov[q]);         // rows >= n and padding columns: zeros
    }
    if (tower == 0 && (MASK || !CAT)) {                                                  // (CAT without MASK: the ACT tile is not used)
#pragma unroll
        for (int q = 0; q < NA; ++q) lds[L8::ACT + er * AP + ej + 32 * q] = av_[q];
    }
    if (tid < 16) {
        float v0 = r0;
        if (tower == 0 && !explicit_adv) v0 = ((r0 - r1) - s0) / s1;                   // ppo2.hpp:401-406
        const bool live = row0 + tid < a.n;
        lds[L8::ROWV + 2 * tid] = live ? v0 : 0.f;
        lds[L8::ROWV + 2 * tid + 1] = live ? r2 : 0.f;
        if constexpr (CAT && !MULTI) { if (tower == 0) lds[L8::MISC + 64 + tid] = rc; }
    }
    if constexpr (MULTI) { if (tower == 0 && tid < 16 * PPO_MAX_COMPONENTS_DEV) lds[L8::MACT + tid] = mk; }    // dead rows, components >= K: zeros, never read
    STAMP(22);
    lds_barrier();
    STAMP(1);
#if T8_PRO >= 2
    load_w_stage<4, 2>(fr[0], W1 + (size_t)t8_stage_row(0, rot) * 256, off_big);
#endif
#if T8_PRO >= 1
    load_w_stage<4, 2>(fr[1], W1 + (size_t)t8_stage_row(1, rot) * 256, off_big);       // behind the barrier: lands while the first layer runs
#endif
#if T8_HEADW == 1
    if (tower == 0) { T8_REQUEST_WHD(); T8_REQUEST_WHT(); }
#endif
    // ---- first layer: h1 = tanh(x W0 + b0), 32 columns per wave ---------------------------------------------------------------------
    {
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        t8_mma_small<2, KS0>(wl0, lds + L8::X0, L8::LD0, c, g, acc);
        const int col = 32 * wave + 2 * c;
        const float b0 = par[net.par_b[0] + col], b1 = par[net.par_b[0] + col + 1];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * g + r;
            float y0 = fast_tanh(acc[0][r] + b0), y1 = fast_tanh(acc[1][r] + b1);
            if (row0 + row >= a.n) { y0 = 0.f; y1 = 0.f; }
            *reinterpret_cast<float2*>(lds + L8::H1 + row * T8_LD + col) = make_float2(y0, y1);
            t8_st_wt2(a.hg[tower][0] + (size_t)(row0 + row) * 256 + col, y0, y1);
        }
    }
    lds_barrier();
    STAMP(2);
    // ---- second layer: h2 = tanh(h1 W1 + b1), K split over the wave pair -------------------------------------------------------------
    {
        f32x4 acc[4];
        t8_big_product(fr, W1, off_big, lds + L8::H1 + 128 * kh, c, g, rot, acc);
        STAMP(11);
#if T8_HEADW == 2
        if (tower == 0) { T8_REQUEST_WHD(); T8_REQUEST_WHT(); }          // in front of the W1^T stages: vector-memory operations return in order, and the head reads these first
#endif
        // the backward product's transposed weights: two stages per wave, in flight through the head and the loss
#if T8_W1T == 0
        load_w_stage<4, 2>(fr[0], W1T + (size_t)t8_stage_row(0, rot) * 256, off_big);
        load_w_stage<4, 2>(fr[1], W1T + (size_t)t8_stage_row(1, rot) * 256, off_big);
#endif
        STAMP(12);
        float out[4][2];
        t8_exchange(acc, lds + L8::D2, p, kh, lane, out);
        STAMP(13);
#if T8_W1T >= 1
        load_w_stage<4, 2>(fr[0], W1T + (size_t)t8_stage_row(0, rot) * 256, off_big);
#endif
#if T8_W1T == 1
        load_w_stage<4, 2>(fr[1], W1T + (size_t)t8_stage_row(1, rot) * 256, off_big);
#endif
        __builtin_amdgcn_sched_barrier(0);
        const int col = 64 * p + 4 * c;
        const float4 b4 = *reinterpret_cast<const float4*>(par + net.par_b[1] + col);
        const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = 4 * g + 2 * kh + i;
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = (row0 + row < a.n) ? fast_tanh(out[j][i] + bb[j]) : 0.f;
            *reinterpret_cast<float4*>(lds + L8::H2 + row * T8_LD + col) = make_float4(y[0], y[1], y[2], y[3]);
            if (tower == 0) st_wt4<T8_WT != 0>(a.hg[0][1] + (size_t)(row0 + row) * 256 + col, make_float4(y[0], y[1], y[2], y[3]));   // (the value head's weight gradient is formed here: nobody reads a copy of its input)
        }
    }
    lds_barrier();
    STAMP(3);
#if T8_W1T == 2
    load_w_stage<4, 2>(fr[1], W1T + (size_t)t8_stage_row(1, rot) * 256, off_big);
    __builtin_amdgcn_sched_barrier(0);
#endif
    // this tower's clip range, hyper[1] = cliprange (policy) or hyper[2] = the value-clip range (vf_loss_row): ONE load, issued where the graph's single
    // cliprange load was (three adjacent words became one dwordx3 whose registers the policy tower then waited for, prefetch included: +4.5 % at configs[2])
    const float cr = a.hyper[tower == 0 ? 1 : 2];
    const float* h2 = lds + L8::H2;
    float* d2 = lds + L8::D2;
    float* misc = lds + L8::MISC;
    if (tower == 0) {
        // ---- policy head: mu = h2 W_mu + b_mu, K split 8 ways, partial tiles meet in LDS (the d2 and d1 tiles are free until the
        // backward products: the exchange of the second layer is behind the barrier above)
        float* scratch = lds + L8::D2;                                                 // [8][16][AP]: 16 or 32 KB of the 33 KB the two tiles span
        static_assert(8 * 16 * AP <= 2 * 16 * T8_LD, "split-K scratch of the policy head");
        {
            f32x4 acc[CTA];
#pragma unroll
            for (int j = 0; j < CTA; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            t8_mma_small<CTA, 2>(whd, h2 + 32 * wave, T8_LD, c, g, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float* dst = scratch + wave * (16 * AP) + (4 * g + r) * AP + CTA * c;
                if constexpr (CTA == 2) *reinterpret_cast<float2*>(dst) = make_float2(acc[0][r], acc[1][r]);
                else *reinterpret_cast<float4*>(dst) = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
            }
        }
        lds_barrier();
        float mu[NA];
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            float s = scratch[er * AP + ej + 32 * q];
#pragma unroll
            for (int w = 1; w < 8; ++w) s += scratch[w * (16 * AP) + er * AP + ej + 32 * q];
            mu[q] = s + par[net.par_bmu + ej + 32 * q];
        }
        STAMP(6);                                                                      // (the scratch lies over d2, which the head's backward product writes: behind the barrier that follows the d mu tile)
        // ---- surrogate loss (G:9428-11290) and its gradient (G:12609-22656): one lane per (row, action) ---------------------------
        const bool live = erow_live;
        float z[NA], sigma[NA], nlp, sent;
        // categorical: ok = the category exists and is allowed; over those, m = max l, a0 = l - m, ex = exp(a0), cz = sum ex, clz = log cz
        bool ok[NA];
        float a0[NA], ex[NA], cz = 1.f, clz = 0.f;
        int cact = -1;
        float zq[NA], lzq[NA], hq[NA];                                                 // MULTI: z, log z and H of the element's OWN component ...
        int actq[NA];                                                                  // ... and that component's action column
        BernParts bp[NA];                                                              // BIN: the element's exp / softplus / probabilities, formed once ...
        float bx[NA];                                                                  // ... and its bit
        if constexpr (MULTI) {
            const int nK = a.comp.K;
            const float* arow = lds + L8::MACT + er * PPO_MAX_COMPONENTS_DEV;
            float mq[NA];
#pragma unroll
            for (int q = 0; q < NA; ++q) {
                ok[q] = ej + 32 * q < nA;
                if constexpr (MASK) ok[q] = ok[q] && (!live || lds[L8::ACT + er * AP + ej + 32 * q] != 0.f);
                mq[q] = 0.f; zq[q] = 1.f; lzq[q] = 0.f; hq[q] = 0.f; actq[q] = -1;
            }
            for (int k = 0; k < nK; ++k) {
                const int o = a.comp.off[k], e = a.comp.off[k + 1];
                float bl = -INFINITY;
#pragma unroll
                for (int q = 0; q < NA; ++q) bl = (ok[q] && ej + 32 * q >= o && ej + 32 * q < e) ? tf_max(bl, mu[q]) : bl;
                const float cm = t8_max32(bl);
#pragma unroll
                for (int q = 0; q < NA; ++q) mq[q] = (ej + 32 * q >= o && ej + 32 * q < e) ? cm : mq[q];
            }
#pragma unroll
            for (int q = 0; q < NA; ++q) { a0[q] = mu[q] - mq[q]; ex[q] = expf(a0[q]); }
            nlp = 0.f; sent = 0.f;
            for (int k = 0; k < nK; ++k) {
                const int o = a.comp.off[k], e = a.comp.off[k + 1];
                const int act = live ? o + (int)arow[k] : -1;                              // compared with column indices only
                float zs = 0.f, las = 0.f, es = 0.f;
#pragma unroll
                for (int q = 0; q < NA; ++q) {
                    const bool in = ok[q] && ej + 32 * q >= o && ej + 32 * q < e;
                    zs += in ? ex[q] : 0.f;
                    las += (in && ej + 32 * q == act) ? a0[q] : 0.f;
                }
                const float kz = t8_sum32(zs);
                const float la = t8_sum32(las);
                const float klz = logf(kz);
#pragma unroll
                for (int q = 0; q < NA; ++q) es += (ok[q] && ej + 32 * q >= o && ej + 32 * q < e) ? cat_entropy_term(ex[q], kz, klz, a0[q]) : 0.f;
                const float hk = t8_sum32(es);
                const float nk = klz - la;
                nlp = k == 0 ? nk : nlp + nk;
                sent = k == 0 ? hk : sent + hk;
#pragma unroll
                for (int q = 0; q < NA; ++q) {
                    const bool mine = ej + 32 * q >= o && ej + 32 * q < e;
                    zq[q] = mine ? kz : zq[q]; lzq[q] = mine ? klz : lzq[q]; hq[q] = mine ? hk : hq[q]; actq[q] = mine ? act : actq[q];
                }
            }
        } else if constexpr (CAT) {
            cact = live ? (int)lds[L8::MISC + 64 + er] : -1;
            float bl = -INFINITY;
#pragma unroll
            for (int q = 0; q < NA; ++q) {
                ok[q] = ej + 32 * q < nA;
                if constexpr (MASK) ok[q] = ok[q] && (!live || lds[L8::ACT + er * AP + ej + 32 * q] != 0.f);
                bl = ok[q] ? tf_max(bl, mu[q]) : bl;
            }
            const float cm = t8_max32(bl);
            float zs = 0.f, las = 0.f, es = 0.f;
#pragma unroll
            for (int q = 0; q < NA; ++q) {
                a0[q] = mu[q] - cm;
                ex[q] = expf(a0[q]);
                zs += ok[q] ? ex[q] : 0.f;
                las += (ok[q] && ej + 32 * q == cact) ? a0[q] : 0.f;                       // the action's a0: one lane's element, zeros elsewhere
            }
            cz = t8_sum32(zs);
            const float la = t8_sum32(las);
            clz = logf(cz);
#pragma unroll
            for (int q = 0; q < NA; ++q) es += ok[q] ? cat_entropy_term(ex[q], cz, clz, a0[q]) : 0.f;
            sent = t8_sum32(es);
            nlp = clz - la;
        } else if constexpr (BIN) {
            float sn = 0.f, se_ = 0.f;
#pragma unroll
            for (int q = 0; q < NA; ++q) {
                const bool lj = ej + 32 * q < nA;
                bp[q] = bern_parts(mu[q]);
                bx[q] = live ? lds[L8::ACT + er * AP + ej + 32 * q] : 0.f;
                sn += lj ? bern_nlp_elem(bp[q], mu[q], bx[q]) : 0.f; se_ += lj ? bern_entropy_elem(bp[q], mu[q]) : 0.f;
            }
            nlp = t8_sum32(sn);
            sent = t8_sum32(se_);
        } else {
            float zz = 0.f, sl_ = 0.f, se_ = 0.f;
#pragma unroll
            for (int q = 0; q < NA; ++q) {
                const bool lj = ej + 32 * q < nA;
                const GaussStd gs = gauss_std(mu[q], par[net.par_ls + ej + 32 * q]);
                sigma[q] = gs.sigma;
                z[q] = gauss_z(live ? lds[L8::ACT + er * AP + ej + 32 * q] : mu[q], mu[q], sigma[q]);
                zz += lj ? z[q] * z[q] : 0.f; sl_ += lj ? gs.logstd : 0.f; se_ += lj ? gauss_entropy_elem(gs.logstd) : 0.f;
            }
            const float ssq = t8_sum32(zz), slog = t8_sum32(sl_);
            sent = t8_sum32(se_);
            nlp = gauss_nlp(ssq, slog, nA);
        }
        const float adv = live ? lds[L8::ROWV + 2 * er] : 0.f;
        const float old_nlp = live ? lds[L8::ROWV + 2 * er + 1] : nlp;
        const SurrogateRow sr = surrogate_row(nlp, old_nlp, adv, cr);
        const float gi = a.inv_n;
        const float d_nlp = surrogate_d_nlp(sr, adv, gi, live);
        if (ej == 0) {
            surrogate_terms(sr, nlp, old_nlp, sent, cr, live, misc, er);
        }
#pragma unroll
        for (int q = 0; q < NA; ++q) {
            float dl = 0.f, dmu = 0.f;
            if constexpr (MULTI) { if (ok[q] && live) dmu = cat_grad_elem(d_nlp, ex[q], zq[q], a0[q], lzq[q], hq[q], ej + 32 * q, actq[q], net.ent_coef, gi); }   // H of j's own component
            else if constexpr (CAT) { if (ok[q] && live) dmu = cat_grad_elem(d_nlp, ex[q], cz, a0[q], clz, sent, ej + 32 * q, cact, net.ent_coef, gi); }   // d l_j; forbidden / padding columns, dead rows: +0
            else if constexpr (BIN) { if (ej + 32 * q < nA && live) dmu = bern_grad_elem(d_nlp, bp[q], mu[q], bx[q], net.ent_coef, gi); }   // d l_j; padding columns, dead rows: +0
            else if (ej + 32 * q < nA && live) gauss_grad_elem(d_nlp, z[q], sigma[q], net.ent_coef, gi, dmu, dl);
            lds[L8::MU + er * L8::LDM + ej + 32 * q] = dmu;                         // the d mu tile: A operand of the head's backward product
            lds[L8::DLS + er * AP + ej + 32 * q] = dl;
            st_wt<false>(a.dmug + (size_t)(row0 + er) * AP + ej + 32 * q, dmu);                   // dead rows / padding columns: zeros
        }
        lds_barrier();
        if (tid < AP) {
            float sb = 0.f, sl = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) { sb += lds[L8::MU + q * L8::LDM + tid]; sl += lds[L8::DLS + q * AP + tid]; }
            st_wt<false>(slot + net.slot_head + tid, sb);
            st_wt<false>(slot + net.slot_aux + tid, sl);
        } else if (tid < AP + 4) {
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) s += misc[q * 4 + (tid - AP)];
            st_wt<false>(slot + net.slot_loss + (tid - AP), s);
        }
        STAMP(7);
        // ---- dY1 = (d mu W_mu^T) .* (1 - h2^2), 32 columns per wave -----------------------------------------------------------------
        {
            f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            t8_mma_small<2, KSA>(whT, lds + L8::MU, L8::LDM, c, g, acc);
            const int col = 32 * wave + 2 * c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * g + r;
                const float2 hh = *reinterpret_cast<const float2*>(h2 + row * T8_LD + col);
                const float y0 = acc[0][r] * (1.0f - hh.x * hh.x), y1 = acc[1][r] * (1.0f - hh.y * hh.y);     // TanhGrad; dead rows: d mu = 0
                *reinterpret_cast<float2*>(d2 + row * T8_LD + col) = make_float2(y0, y1);
                t8_st_wt2(a.dyg[0][1] + (size_t)(row0 + row) * 256 + col, y0, y1);
            }
        }
    } else {
        // ---- value head + clipped value loss (G:10213-10837) and its gradient (G:14975-19571): 32 lanes per row ---------------------
        const float voff = a.hyper[3];
        const float* wv = par + net.par_wv;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) s = fmaf(h2[er * T8_LD + ej + 32 * k], wv[ej + 32 * k], s);
        const float v = t8_sum32(s) + par[net.par_bv];
        float dv = 0.f, lossv = 0.f;
        if (erow_live) {
            const float R = lds[L8::ROWV + 2 * er], vo = lds[L8::ROWV + 2 * er + 1];
            vf_loss_row(v, R, vo, cr, voff, net.vf_coef * 0.5f * a.inv_n, lossv, dv);
        }
        if (ej == 0) { misc[er] = dv; misc[16 + er] = lossv; }
        lds_barrier();
        STAMP(7);
        if (tid == 0) {
            float sb = 0.f, sl = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) { sb += misc[q]; sl += misc[16 + q]; }
            st_wt<false>(slot + net.slot_aux, sb);            // db_v
            st_wt<false>(slot + net.slot_loss, sl);           // sum of max((v-R)^2, (vclip-R)^2)
        }
        // dW_v[k] = sum_rows h2[row,k] dv[row] ; dY1 = dv (x) w_v .* (1 - h2^2): thread (k = tid & 255, rows 8 (tid >> 8) .. + 7)
        {
            const int k = tid & 255, q0 = (tid >> 8) * 8;
            const float w = wv[k];
            if (tid < 256) {
                float sw = 0.f;
#pragma unroll
                for (int q = 0; q < 16; ++q) sw = fmaf(h2[q * T8_LD + k], misc[q], sw);
                st_wt<false>(slot + net.slot_head + k, sw);
            }
#pragma unroll
            for (int q = q0; q < q0 + 8; ++q) {
                const float h = h2[q * T8_LD + k];
                const float d = (misc[q] * w) * (1.0f - h * h);
                d2[q * T8_LD + k] = d;
                st_wt<T8_WT != 0>(a.dyg[1][1] + (size_t)(row0 + q) * 256 + k, d);             // dead rows: d == 0
            }
        }
    }
    lds_barrier();
    STAMP(8);
    // ---- dY0 = (dY1 W1^T) .* (1 - h1^2), K split over the wave pair (the h2 tile is free now: exchange scratch) ------------------------
    {
        f32x4 acc[4];
        t8_big_product(fr, W1T, off_big, d2 + 128 * kh, c, g, rot, acc);
        STAMP(14);
        float out[4][2];
        t8_exchange(acc, lds + L8::H2, p, kh, lane, out);
        STAMP(15);
        const int col = 64 * p + 4 * c;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = 4 * g + 2 * kh + i;
            const float4 hh = *reinterpret_cast<const float4*>(lds + L8::H1 + row * T8_LD + col);
            const float4 y = make_float4(out[0][i] * (1.0f - hh.x * hh.x), out[1][i] * (1.0f - hh.y * hh.y), out[2][i] * (1.0f - hh.z * hh.z), out[3][i] * (1.0f - hh.w * hh.w));
            *reinterpret_cast<float4*>(lds + L8::D1 + row * T8_LD + col) = y;
            st_wt4<T8_WT != 0>(a.dyg[tower][0] + (size_t)(row0 + row) * 256 + col, y);
        }
    }
    lds_barrier();
    STAMP(9);
    // ---- bias gradients: db1 = sum_rows dY1 (threads 0..255), db0 = sum_rows dY0 (threads 256..511)  (.../Add_grad/Sum_1) -------------
    {
        const int k = tid & 255;
        const float* src = (tid < 256) ? d2 : lds + L8::D1;
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) s += src[q * T8_LD + k];
        st_wt<false>(slot + net.slot_db[tid < 256 ? 1 : 0] + k, s);
    }
    STAMP(10);
#undef T8_REQUEST_WHD
#undef T8_REQUEST_WHT
}

template <int KP0, int AP>
__global__ __launch_bounds__(T8_THREADS) void train8_kernel(NetDev net, TrainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    warm_kernargs<sizeof(NetDev) + sizeof(TrainArgs)>();
    train8_body<KP0, AP>(net, a, lds, blockIdx.x, blockIdx.y, gridDim.x);
}
// the categorical forms, train8_kernel<KP0, AP, CAT, MASK>: an OVERLOAD, not two defaulted parameters of the template above -- the Gaussian kernels keep their
// symbols (and tools/kernel_code_diff.py pairs them with every earlier build's)
template <int KP0, int AP, bool CAT, bool MASK>
__global__ __launch_bounds__(T8_THREADS) void train8_kernel(NetDev net, TrainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    warm_kernargs<sizeof(NetDev) + sizeof(TrainArgs)>();
    train8_body<KP0, AP, CAT, MASK>(net, a, lds, blockIdx.x, blockIdx.y, gridDim.x);
}
// the multi-categorical forms, train8_kernel<KP0, AP, CAT, MASK, MULTI>: a further overload that takes the component table behind the arguments; T8L::TOTAL_M floats
// of dynamic LDS (the action rows' region lies behind the carve of the other forms)
template <int KP0, int AP, bool CAT, bool MASK, bool MULTI>
__global__ __launch_bounds__(T8_THREADS) void train8_kernel(NetDev net, TrainArgsM a) {
    static_assert(MULTI && CAT, "the multi-categorical overload: a form of the categorical head");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    warm_kernargs<sizeof(NetDev) + sizeof(TrainArgsM)>();
    train8_body<KP0, AP, CAT, MASK, MULTI>(net, a, lds, blockIdx.x, blockIdx.y, gridDim.x);
}
// the multi-binary form, train8_kernel<KP0, AP, MbinHead>: an overload with a head TYPE on the Gaussian arguments under a type of their own (TrainArgsB), as
// train_fwd_bwd_kernel / narrow_train_kernel<.., MbinHead> are -- every other instantiation keeps its symbol.  The other forms' carve and dynamic LDS (T8L::TOTAL).
template <int KP0, int AP, class HEAD>
__global__ __launch_bounds__(T8_THREADS) void train8_kernel(NetDev net, TrainArgsB a) {
    static_assert(std::is_same_v<HEAD, MbinHead>, "the overload with a head TYPE is the multi-binary head's");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    warm_kernargs<sizeof(NetDev) + sizeof(TrainArgsB)>();
    train8_body<KP0, AP, false, false, false, true>(net, a, lds, blockIdx.x, blockIdx.y, gridDim.x);
}

// The forms launched while target-KL early stopping is on (update_stopped, ppo_kernels.hpp): the kernels above behind the entry check.  Kernels of their own, so that
// the ones a handle launches with the setting off stay what they were.
template <int KP0, int AP>
__global__ __launch_bounds__(T8_THREADS) void train8_stop_kernel(NetDev net, TrainArgs a, const unsigned* stop) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    warm_kernargs<sizeof(NetDev) + sizeof(TrainArgs) + sizeof(stop)>();
    if (update_stopped(stop)) return;
    train8_body<KP0, AP>(net, a, lds, blockIdx.x, blockIdx.y, gridDim.x);
}
template <int KP0, int AP, bool CAT, bool MASK>
__global__ __launch_bounds__(T8_THREADS) void train8_stop_kernel(NetDev net, TrainArgs a, const unsigned* stop) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    warm_kernargs<sizeof(NetDev) + sizeof(TrainArgs) + sizeof(stop)>();
    if (update_stopped(stop)) return;
    train8_body<KP0, AP, CAT, MASK>(net, a, lds, blockIdx.x, blockIdx.y, gridDim.x);
}
template <int KP0, int AP, bool CAT, bool MASK, bool MULTI>
__global__ __launch_bounds__(T8_THREADS) void train8_stop_kernel(NetDev net, TrainArgsM a, const unsigned* stop) {
    static_assert(MULTI && CAT, "the multi-categorical overload: a form of the categorical head");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    warm_kernargs<sizeof(NetDev) + sizeof(TrainArgsM) + sizeof(stop)>();
    if (update_stopped(stop)) return;
    train8_body<KP0, AP, CAT, MASK, MULTI>(net, a, lds, blockIdx.x, blockIdx.y, gridDim.x);
}
template <int KP0, int AP, class HEAD>
__global__ __launch_bounds__(T8_THREADS) void train8_stop_kernel(NetDev net, TrainArgsB a, const unsigned* stop) {
    static_assert(std::is_same_v<HEAD, MbinHead>, "the overload with a head TYPE is the multi-binary head's");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    warm_kernargs<sizeof(NetDev) + sizeof(TrainArgsB) + sizeof(stop)>();
    if (update_stopped(stop)) return;
    train8_body<KP0, AP, false, false, false, true>(net, a, lds, blockIdx.x, blockIdx.y, gridDim.x);
}
