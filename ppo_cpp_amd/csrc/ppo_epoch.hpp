// ppo_epoch.hpp -- the ONE home of the update preparation: the epoch shuffle (position of the permuted order -> source row -> storage row), the two-pass
// advantage statistics of a minibatch, the gather of an epoch into minibatch order, and the GAE scans in front of them.  Every statement that several kernels
// share is a `__device__ __forceinline__` piece here; the kernels keep their loops, their LDS blocks and their barriers' places and call the pieces inside them
// (the only pieces with a loop are shuffle_row's cycle walk and gae_scan).  The build does not contract (-ffp-contract=off), so every site gets the bits of
// the expression written out in place; tests/test_hip_parity.py (test_epoch_advantages_are_bitwise_adv_normalize) holds the statistics of the epoch
// kernels against adv_normalize_kernel's as bytes.
// As with ppo_head.hpp and ppo_envnorm.hpp a piece should leave its kernels' machine code alone (tools/kernel_code_diff.py).  Three kernels moved (operands of
// the walk's multiply swapped, two instructions reordered, one more mask instruction in epoch_prepare_gather_kernel; no figure changed); two sites stay written
// out and say why: epoch_prepare_kernel's world > 1 branch and the gae_long pair (profiles/EXPERIMENTS.md).
// Included by ppo_kernels.hpp (after wave_sum_lane0), which every other header sees.
#pragma once

// ------------------------------------------------------------------------------------------------------------
// Epoch preparation (ppo2.hpp:274-307 + 401-406).  Block k handles minibatch k of the epoch:
//   r    = flattened env-major source row that lands at permuted position k*M + i   (inverse permutation)
//   gidx = its time-major storage row (runner.hpp:136-152: r = e*T + t  ->  t*E + e)
//   stats[k] = { mean(adv), sqrt(mean((adv-mean)^2)) + 1e-8 }  with adv = returns - values
// inv_perm == null: a keyed bijection on [0,B) (multiply-xorshift rounds + cycle walking) plays the shuffle.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t keyed_bijection(uint32_t x, uint32_t bits, uint32_t mask, uint32_t k0, uint32_t k1) {
    const uint32_t sh = bits > 1 ? bits / 2 : 1;
    x = (x * (k0 | 1u) + k1) & mask;  x ^= x >> sh;
    x = (x * 0x9E3779B1u + (k0 >> 7)) & mask;  x ^= x >> sh;
    x = (x * (k1 | 1u) + 0x85EBCA6Bu) & mask;  x ^= x >> sh;
    x = (x * 0xC2B2AE35u + k0) & mask;  x ^= x >> sh;
    return x;
}

struct EpochArgs {
    const int* inv_perm;     // [B] or null
    const uint32_t* keys;    // {k0, k1} of this epoch (device memory: a replayed graph must see fresh keys)
    uint32_t bits;
    int B, M, T, E;
    const float* returns; const float* values;   // [T*E] storage order
    int* gidx;               // [B]
    float* stats;            // [B/M][2]
    int phase;               // 0: single rank, everything ; data parallel: 1 index + local sums, 2 local squared deviations, 3 finish
    float* xch;              // two vectors of B/M partial sums all-reduced by the host between the phases; the second starts at xch2
    int xch2;                // (a multiple of 4 floats: the peer all-reduce reads its source as 16-byte vectors)
    float n_global;          // minibatch rows over all ranks
    // literal data-parallel sampling (ppo_dist_global_shuffle): ONE permutation of the B * world rows of all ranks; returns / values
    // are the all-gathered [world][T][E] arrays, this rank trains rows [k Mg + rank M, k Mg + (rank + 1) M) of global minibatch k
    int world, rank;         // world > 1 selects this mode (phase 0: the statistics of the whole minibatch are computed locally)
};

// ---- the pieces: the shuffle ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t shuffle_mask(uint32_t bits) { return (bits >= 32) ? 0xFFFFFFFFu : ((1u << bits) - 1u); }
// the flattened env-major source row at position pos of the permuted order of n rows: the explicit inverse permutation, or the cycle walk of the bijection
__device__ __forceinline__ int shuffle_row(const EpochArgs& a, uint32_t mask, int pos, int n) {
    if (a.inv_perm) return a.inv_perm[pos];
    uint32_t x = (uint32_t)pos;
    do { x = keyed_bijection(x, a.bits, mask, a.keys[0], a.keys[1]); } while (x >= (uint32_t)n);
    return (int)x;
}
// r = e * T + t -> its time-major storage row t * E + e; and with the rows of ALL ranks in one permutation (r = e_global * T + t: rank e_global / E owns it)
// its place [rank][t][e] in the all-gathered arrays.  (The second equals the first while r < T * E.)
__device__ __forceinline__ int storage_row(int r, int T, int E) { return (r % T) * E + (r / T); }
__device__ __forceinline__ int storage_row_gathered(int r, int T, int E) {
    const int eg = r / T, t = r - eg * T, rs = eg / E, e = eg - rs * E;
    return rs * (T * E) + t * E + e;
}

// ---- the pieces: the advantage statistics (ppo2.hpp:401-406) ----------------------------------------------------------------------------------------------
// Both passes of a 1024-thread workgroup end the same way: block_park leaves every wave's sum in red[] (SYNC_BEFORE: the second pass, whose red[] the first
// pass' thread 0 may still be reading), and after its barrier thread 0 adds them in index order with parked_total.  mean = total / n, then
// den = adv_den(total of the squared deviations, n); an advantage is adv_normalized(R, V, mean, den).
#define EP_THREADS 1024             // one workgroup per minibatch: its M rows spread over 16 waves (256 threads left 16 rows per thread
                                    // in two dependent passes: 13.6 us per epoch at M = 2048)
template <bool SYNC_BEFORE>
__device__ __forceinline__ void block_park(float v, float* red, int tid) {
    v = wave_sum_lane0(v);
    if constexpr (SYNC_BEFORE) __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
}
__device__ __forceinline__ float parked_total(const float* red) {
    float tot = 0.f;
    for (int w = 0; w < EP_THREADS / 64; ++w) tot += red[w];           // fixed order
    return tot;
}
__device__ __forceinline__ float adv_den(float tot, float n) { return (float)((double)sqrtf(tot / n) + 1e-8); }
__device__ __forceinline__ float adv_normalized(float R, float V, float mean, float den) { return ((R - V) - mean) / den; }

// The world > 1 branch stays beside the single-rank passes, both built from the pieces: folded into one (row count, row lookup and gidx write selected per row)
// the kernel needs 58 scalar registers instead of 54, and with the passes as one template piece over the mode 56.
__global__ __launch_bounds__(EP_THREADS) void epoch_prepare_kernel(EpochArgs a) {
    __shared__ float red[EP_THREADS / 64];
    __shared__ float s_mean;
    const int k = blockIdx.x, tid = threadIdx.x;
    if (a.phase == 3) {
        if (tid == 0) {
            a.stats[2 * k] = a.xch[k] / a.n_global;
            a.stats[2 * k + 1] = adv_den(a.xch[a.xch2 + k], a.n_global);
        }
        return;
    }
    const uint32_t mask = shuffle_mask(a.bits);
    if (a.world > 1) {
        // one global permutation (ppo2.hpp:288-307 applied to the rows of ALL ranks): only this rank's M rows of the global minibatch go into gidx, so the
        // second pass derives the rows again
        const int Bg = a.B * a.world, Mg = a.M * a.world;
        auto src_of = [&](int posg) __attribute__((always_inline)) { return storage_row_gathered(shuffle_row(a, mask, posg, Bg), a.T, a.E); };
        float sum = 0.f;
        for (int i = tid; i < Mg; i += EP_THREADS) {
            const int s = src_of(k * Mg + i);
            const int li = i - a.rank * a.M;
            if (li >= 0 && li < a.M) a.gidx[k * a.M + li] = s;
            sum += a.returns[s] - a.values[s];
        }
        block_park<false>(sum, red, tid);
        if (tid == 0) s_mean = parked_total(red) / (float)Mg;
        __syncthreads();
        const float mean = s_mean;
        float sq = 0.f;
        for (int i = tid; i < Mg; i += EP_THREADS) {
            const int s = src_of(k * Mg + i);
            const float d = (a.returns[s] - a.values[s]) - mean;
            sq += d * d;
        }
        block_park<true>(sq, red, tid);
        if (tid == 0) { a.stats[2 * k] = mean; a.stats[2 * k + 1] = adv_den(parked_total(red), (float)Mg); }
        return;
    }
    float sum = 0.f;
    if (a.phase != 2) {
        for (int i = tid; i < a.M; i += EP_THREADS) {
            const int pos = k * a.M + i;
            const int s = storage_row(shuffle_row(a, mask, pos, a.B), a.T, a.E);
            a.gidx[pos] = s;
            sum += a.returns[s] - a.values[s];
        }
        block_park<false>(sum, red, tid);
        if (tid == 0) {
            const float tot = parked_total(red);
            s_mean = tot / (float)a.M;
            if (a.phase == 1) a.xch[k] = tot;
        }
        __syncthreads();
        if (a.phase == 1) return;
    } else {
        if (tid == 0) s_mean = a.xch[k] / a.n_global;      // global mean of this minibatch
        __syncthreads();
    }
    const float mean = s_mean;
    float sq = 0.f;
    for (int i = tid; i < a.M; i += EP_THREADS) {
        const int s = a.gidx[k * a.M + i];
        const float d = (a.returns[s] - a.values[s]) - mean;
        sq += d * d;
    }
    block_park<true>(sq, red, tid);
    if (tid == 0) {
        const float tot = parked_total(red);
        if (a.phase == 2) a.xch[a.xch2 + k] = tot;
        else { a.stats[2 * k] = mean; a.stats[2 * k + 1] = adv_den(tot, (float)a.M); }
    }
}

// Materialise the permuted epoch (the reference's `perm * v` copies, ppo2.hpp:291-296) in minibatch order so that the
// train kernel reads contiguous rows with no index indirection: 16 rows per block; advantages are normalised here
// with the minibatch statistics of epoch_prepare_kernel.
struct GatherArgs {
    const int* gidx; const float* stats; int B, M, O, A;
    const float* obs; const float* act; const float* ret; const float* val; const float* nlp;
    float* mb_obs; float* mb_act; float* mb_adv; float* mb_ret; float* mb_val; float* mb_nlp;
#ifdef PPO_STAMPS
    unsigned long long* stamps;
#endif
    const float* mask; float* mb_mask; int Am;     // action masks [B, Am] -> minibatch order: the <MASK> instantiations only (a masking handle)
};

// ---- the pieces: a gathered row's scalar fields; the 16-row gathers' index prologue and scalar tail -------------------------------------------------------
__device__ __forceinline__ void gather_row_scalars(const GatherArgs& a, int p, int s, float R, float V, const float& mean, const float& den) {
    a.mb_ret[p] = R; a.mb_val[p] = V; a.mb_nlp[p] = a.nlp[s];
    a.mb_adv[p] = adv_normalized(R, V, mean, den);                              // ppo2.hpp:401-406 (mean, den are read here, behind the three stores)
}
__device__ __forceinline__ void gather16_src(const GatherArgs& a, int* src, int pos0, int tid) {
    if (tid < 16 && pos0 + tid < a.B) src[tid] = a.gidx[pos0 + tid];
    __syncthreads();
}
__device__ __forceinline__ void gather16_scalars(const GatherArgs& a, const int* src, int pos0, int tid) {
    if (tid < 16 && pos0 + tid < a.B) {
        const int p = pos0 + tid, s = src[tid], k = p / a.M;
        gather_row_scalars(a, p, s, a.ret[s], a.val[s], a.stats[2 * k], a.stats[2 * k + 1]);
    }
}

template <bool MASK = false>
__global__ __launch_bounds__(256) void epoch_gather_kernel(GatherArgs a) {
    __shared__ int src[16];
    const int pos0 = blockIdx.x * 16, tid = threadIdx.x;
    gather16_src(a, src, pos0, tid);
    const int W = a.O + a.A;
    for (int i = tid; i < 16 * W; i += 256) {
        const int r = i / W, j = i - r * W;
        if (pos0 + r >= a.B) continue;
        if (j < a.O) a.mb_obs[(size_t)(pos0 + r) * a.O + j] = a.obs[(size_t)src[r] * a.O + j];
        else a.mb_act[(size_t)(pos0 + r) * a.A + (j - a.O)] = a.act[(size_t)src[r] * a.A + (j - a.O)];
    }
    if constexpr (MASK) {
        for (int i = tid; i < 16 * a.Am; i += 256) {
            const int r = i / a.Am, j = i - r * a.Am;
            if (pos0 + r < a.B) a.mb_mask[(size_t)(pos0 + r) * a.Am + j] = a.mask[(size_t)src[r] * a.Am + j];
        }
    }
    gather16_scalars(a, src, pos0, tid);
}

// The same gather for observation / action widths that are multiples of 4 (configs[4]: 256 / 64), 16 bytes per access (a wave instruction of the element-wise form
// touches 64 x 4 bytes of 1 - 2 rows; this one 64 x 16), and -- bf16 path -- the observations written ONCE, as the bf16 operand rows the GEMMs read (X [B][Kp0]; the
// padding columns of a row are never written and stay zero): the fp32 copy of the epoch and the staging launch behind it (read it again, write bf16) go away.
// 16 rows per workgroup as above; same values, same statistics.
struct Gather4Args { GatherArgs g; __bf16* xe; int Kp0; };
__global__ __launch_bounds__(256) void epoch_gather4_kernel(Gather4Args q) {
    const GatherArgs& a = q.g;
    __shared__ int src[16];
    const int pos0 = blockIdx.x * 16, tid = threadIdx.x;
    gather16_src(a, src, pos0, tid);
    const int QO = a.O >> 2, QW = (a.O + a.A) >> 2;
    typedef __bf16 bf16q_t __attribute__((ext_vector_type(4)));
    for (int i = tid; i < 16 * QW; i += 256) {
        const int r = i / QW, jq = i - r * QW;
        if (pos0 + r >= a.B) continue;
        if (jq < QO) {
            const float4 v = *reinterpret_cast<const float4*>(a.obs + (size_t)src[r] * a.O + 4 * jq);
            if (q.xe) { bf16q_t o; o[0] = (__bf16)v.x; o[1] = (__bf16)v.y; o[2] = (__bf16)v.z; o[3] = (__bf16)v.w; *reinterpret_cast<bf16q_t*>(q.xe + (size_t)(pos0 + r) * q.Kp0 + 4 * jq) = o; }
            else *reinterpret_cast<float4*>(a.mb_obs + (size_t)(pos0 + r) * a.O + 4 * jq) = v;
        } else {
            const int ja = 4 * (jq - QO);
            *reinterpret_cast<float4*>(a.mb_act + (size_t)(pos0 + r) * a.A + ja) = *reinterpret_cast<const float4*>(a.act + (size_t)src[r] * a.A + ja);
        }
    }
    gather16_scalars(a, src, pos0, tid);
}

// epoch_prepare_kernel (single rank, local shuffle) AND epoch_gather_kernel in one launch: EPG_SPLIT workgroups per minibatch each derive the
// minibatch's index map and advantage statistics (through the same pieces in the same order, so every one of them holds the same bits; the redundant
// work is a few thousand integer hashes) and then copy their 1 / EPG_SPLIT share of its rows.  One launch and one dependent round trip through
// memory (the index map) per epoch less: the map never leaves the workgroup's LDS except as this epoch's `gidx` record.
#define EPG_SPLIT 8
#define EPG_MAX_M 8192              // rows of a minibatch the LDS copy of the index map holds (32 KB)
template <bool MASK = false>
__global__ __launch_bounds__(EP_THREADS) void epoch_prepare_gather_kernel(EpochArgs a, GatherArgs ga) {
    __shared__ float red[EP_THREADS / 64];
    __shared__ float s_mean, s_den;
    __shared__ int s_idx[EPG_MAX_M];
    __shared__ float s_rv[2 * ((EPG_MAX_M + EPG_SPLIT - 1) / EPG_SPLIT)];       // returns | values of this workgroup's own rows (met in the first pass)
#ifdef PPO_STAMPS
#define ESTAMP(i) do { if (ga.stamps && threadIdx.x == 0) ga.stamps[(size_t)blockIdx.x * 8 + (i)] = __builtin_readcyclecounter(); } while (0)
#else
#define ESTAMP(i) do { } while (0)
#endif
    ESTAMP(0);
    const int k = blockIdx.x / EPG_SPLIT, part = blockIdx.x % EPG_SPLIT, tid = threadIdx.x;
    const uint32_t mask = shuffle_mask(a.bits);
    const int per = (a.M + EPG_SPLIT - 1) / EPG_SPLIT, r0 = part * per, r1 = min(a.M, r0 + per);
    // In-kernel stamps (tools/stamps_epoch.py): of this kernel's 36 k cycles, 6.6 k were the second pass gathering again what the first had
    // seen (a scattered 4-byte gather is 64 cache-line lookups per wave instruction) and 3 k the scalar fields' own gathers.  A thread's
    // advantages now stay in registers between the passes and the rows this workgroup copies leave their returns / values in LDS when the
    // first pass meets them: 25 k cycles, 17.5 -> 13 us.  (Measured without effect on the 9 k-cycle row copy: all its loads ahead of its
    // stores, 8-byte elements, shifts instead of the divisions -- it waits for scattered rows, not for instructions.)
    constexpr int RU = EPG_MAX_M / EP_THREADS;                                  // advantages per thread held in registers
    float adv[RU];
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < RU; ++u) {
        const int i = tid + EP_THREADS * u;
        adv[u] = 0.f;
        if (i < a.M) {
            const int pos = k * a.M + i;
            const int s = storage_row(shuffle_row(a, mask, pos, a.B), a.T, a.E);
            s_idx[i] = s;
            if (part == 0) a.gidx[pos] = s;
            const float R = a.returns[s], V = a.values[s];
            if (i >= r0 && i < r1) { s_rv[2 * (i - r0)] = R; s_rv[2 * (i - r0) + 1] = V; }
            adv[u] = R - V;
            sum += adv[u];
        }
    }
    ESTAMP(1);
    block_park<false>(sum, red, tid);
    if (tid == 0) s_mean = parked_total(red) / (float)a.M;
    __syncthreads();
    ESTAMP(2);
    const float mean = s_mean;
    float sq = 0.f;
#pragma unroll
    for (int u = 0; u < RU; ++u) {
        if (tid + EP_THREADS * u < a.M) { const float d = adv[u] - mean; sq += d * d; }
    }
    ESTAMP(3);
    block_park<true>(sq, red, tid);
    if (tid == 0) {
        s_den = adv_den(parked_total(red), (float)a.M);
        if (part == 0) { a.stats[2 * k] = mean; a.stats[2 * k + 1] = s_den; }
    }
    __syncthreads();
    ESTAMP(4);
    const float den = s_den;
    // ---- this workgroup's rows of the minibatch: [r0, r1) --------------------------------------------------------------------------------
    const int W = ga.O + ga.A, total = (r1 - r0) * W;
    int rr = tid / W, jj = tid - rr * W;                                        // element tid of the [rows][W] block; then + EP_THREADS per sweep
    const int dq = EP_THREADS / W, dr = EP_THREADS - dq * W;
    for (int i = tid; i < total; i += EP_THREADS) {
        const int r = r0 + rr, p = k * a.M + r, s = s_idx[r];
        if (jj < ga.O) ga.mb_obs[(size_t)p * ga.O + jj] = ga.obs[(size_t)s * ga.O + jj];
        else ga.mb_act[(size_t)p * ga.A + (jj - ga.O)] = ga.act[(size_t)s * ga.A + (jj - ga.O)];
        rr += dq; jj += dr;
        if (jj >= W) { jj -= W; ++rr; }
    }
    if constexpr (MASK) {
        for (int i = tid; i < (r1 - r0) * ga.Am; i += EP_THREADS) {
            const int r = r0 + i / ga.Am, j = i % ga.Am;
            ga.mb_mask[(size_t)(k * a.M + r) * ga.Am + j] = ga.mask[(size_t)s_idx[r] * ga.Am + j];
        }
    }
    ESTAMP(5);
    for (int r = r0 + tid; r < r1; r += EP_THREADS)
        gather_row_scalars(ga, k * a.M + r, s_idx[r], s_rv[2 * (r - r0)], s_rv[2 * (r - r0) + 1], mean, den);
    ESTAMP(6);
#ifdef PPO_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ESTAMP(7);
#endif
}

// inv[perm[i]] = i   (out.row(perm[i]) = in.row(i), ppo2.hpp:291-296)
__global__ void invert_perm_kernel(const int* perm, int* inv, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) inv[perm[i]] = i;
}

// standalone advantage normalisation of an explicit minibatch (ppo2.hpp:401-406), single block: the epoch kernels' two passes over rows 0 .. n-1 in place
__global__ __launch_bounds__(EP_THREADS) void adv_normalize_kernel(const float* returns, const float* values, int n, float* advs) {
    __shared__ float red[EP_THREADS / 64];
    __shared__ float s_val;
    const int tid = threadIdx.x;
    float sum = 0.f;
    for (int i = tid; i < n; i += EP_THREADS) sum += returns[i] - values[i];
    block_park<false>(sum, red, tid);
    if (tid == 0) s_val = parked_total(red) / (float)n;
    __syncthreads();
    const float mean = s_val;
    float sq = 0.f;
    for (int i = tid; i < n; i += EP_THREADS) { const float d = (returns[i] - values[i]) - mean; sq += d * d; }
    block_park<true>(sq, red, tid);
    if (tid == 0) s_val = adv_den(parked_total(red), (float)n);
    __syncthreads();
    const float denom = s_val;
    for (int i = tid; i < n; i += EP_THREADS) advs[i] = adv_normalized(returns[i], values[i], mean, denom);
}

// ------------------------------------------------------------------------------------------------------------
// GAE(lambda) (runner.hpp:159-191): one thread per env, serial in t, coalesced across envs (time-major buffers).
// TRUNC: with a value bootstrap at time-limit truncations (no reference counterpart: Runner::set_returns treats every done as
// terminal).  tv [T,E] holds V(terminal observation) on the rows whose step was cut by a time limit and 0 elsewhere; the reward of
// such a row becomes rewards + gamma tv, everything else -- nnt = 1 - done, so the lambda trace is still cut at the episode
// boundary -- is the plain scan:
//   delta_t = (rewards[t] + gamma tv[t]) + gamma V[t+1] (1 - done[t+1]) - V[t]
// With tv == 0 the results equal the plain scan's (x + gamma * 0 == x for every finite x, -0 aside).
// One body, the flag around that term, and entry points that keep their names and parameter lists: the plain instantiation never sees tv.  That
// gae_kernel (and gae_trunc_kernel) kept their code bit for bit is what tools/kernel_code_diff.py shows against the commit that still had two
// written-out copies (profiles/EXPERIMENTS.md), where care on every edit used to be the guarantee.
// ------------------------------------------------------------------------------------------------------------
template <bool TRUNC>
__device__ __forceinline__ float gae_reward(const float* rewards, const float* tv, size_t i, float gamma) {
    if constexpr (TRUNC) return rewards[i] + gamma * tv[i];
    else return rewards[i];
}
template <bool TRUNC>
__device__ __forceinline__ void gae_scan(const float* rewards, const float* values, const float* dones, const float* last_values,
                                         const float* last_dones, const float* tv, int T, int E, float gamma, float lam, float* returns) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    float last = 0.f;
    float nv = last_values[e];
    float nnt = 1.0f - last_dones[e];
    for (int t = T - 1; t >= 0; --t) {
        const size_t i = (size_t)t * E + e;
        const float v = values[i];
        const float delta = gae_reward<TRUNC>(rewards, tv, i, gamma) + gamma * (nv * nnt) - v;
        last = delta + (gamma * lam) * (nnt * last);
        returns[i] = last + v;
        nv = v;
        nnt = 1.0f - dones[i];
    }
}
__global__ void gae_kernel(const float* rewards, const float* values, const float* dones, const float* last_values,
                           const float* last_dones, int T, int E, float gamma, float lam, float* returns) {
    gae_scan<false>(rewards, values, dones, last_values, last_dones, nullptr, T, E, gamma, lam, returns);
}
__global__ void gae_trunc_kernel(const float* rewards, const float* values, const float* dones, const float* last_values,
                                 const float* last_dones, const float* tv, int T, int E, float gamma, float lam, float* returns) {
    gae_scan<true>(rewards, values, dones, last_values, last_dones, tv, T, E, gamma, lam, returns);
}

// Few environments, long rollouts (the reference's own command line: ONE env x 2048 steps): the scan above is 2048 dependent
// iterations of global loads on one lane (280 us).  One workgroup per env: every temporal-difference term delta_t and every
// continuation flag are formed by all threads in parallel (the same expressions on the same operands) and parked in LDS; one lane then
// runs the recurrence last = delta_t + (gamma lam) (nnt_t last) -- two dependent operations per step, its operands read ahead.
// Bit-identical to gae_kernel (same operations in the same order per element).
// This form and its truncation sibling below stay two written-out kernels: as gae_long_scan<TRUNC>, whole or with either loop as a piece, the serial lane's loops
// are laid out otherwise (405 -> 410 instructions, 38 -> 40 scalar registers in gae_long_kernel)
#define GAE_LONG_THREADS 256
__global__ __launch_bounds__(GAE_LONG_THREADS) void gae_long_kernel(const float* rewards, const float* values, const float* dones, const float* last_values,
                                                                   const float* last_dones, int T, int E, float gamma, float lam, float* returns) {
    extern __shared__ __attribute__((aligned(16))) float gl_lds[];
    float* s_delta = gl_lds; float* s_nnt = gl_lds + T; float* s_v = gl_lds + 2 * T;
    const int e = blockIdx.x;
    for (int t = threadIdx.x; t < T; t += GAE_LONG_THREADS) {
        const size_t i = (size_t)t * E + e;
        const float v = values[i];
        const float nv = t == T - 1 ? last_values[e] : values[i + E];
        const float nnt = 1.0f - (t == T - 1 ? last_dones[e] : dones[i + E]);
        s_delta[t] = rewards[i] + gamma * (nv * nnt) - v;
        s_nnt[t] = nnt; s_v[t] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float last = 0.f;
        const float gl = gamma * lam;
        int t = T - 1;
        for (; t >= 7; t -= 8) {
            float d[8], n[8], v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { d[k] = s_delta[t - k]; n[k] = s_nnt[t - k]; v[k] = s_v[t - k]; }
#pragma unroll
            for (int k = 0; k < 8; ++k) { last = d[k] + gl * (n[k] * last); s_delta[t - k] = last + v[k]; }
        }
        for (; t >= 0; --t) { last = s_delta[t] + gl * (s_nnt[t] * last); s_delta[t] = last + s_v[t]; }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += GAE_LONG_THREADS) returns[(size_t)t * E + e] = s_delta[t];
}

// ... with the bootstrap term folded into s_delta[t] in the parallel phase, so the serial lane and the 3T floats of LDS are gae_long_kernel's
__global__ __launch_bounds__(GAE_LONG_THREADS) void gae_long_trunc_kernel(const float* rewards, const float* values, const float* dones, const float* last_values,
                                                                         const float* last_dones, const float* tv, int T, int E, float gamma, float lam, float* returns) {
    extern __shared__ __attribute__((aligned(16))) float gl_lds[];
    float* s_delta = gl_lds; float* s_nnt = gl_lds + T; float* s_v = gl_lds + 2 * T;
    const int e = blockIdx.x;
    for (int t = threadIdx.x; t < T; t += GAE_LONG_THREADS) {
        const size_t i = (size_t)t * E + e;
        const float v = values[i];
        const float nv = t == T - 1 ? last_values[e] : values[i + E];
        const float nnt = 1.0f - (t == T - 1 ? last_dones[e] : dones[i + E]);
        s_delta[t] = (rewards[i] + gamma * tv[i]) + gamma * (nv * nnt) - v;
        s_nnt[t] = nnt; s_v[t] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float last = 0.f;
        const float gl = gamma * lam;
        int t = T - 1;
        for (; t >= 7; t -= 8) {
            float d[8], n[8], v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { d[k] = s_delta[t - k]; n[k] = s_nnt[t - k]; v[k] = s_v[t - k]; }
#pragma unroll
            for (int k = 0; k < 8; ++k) { last = d[k] + gl * (n[k] * last); s_delta[t - k] = last + v[k]; }
        }
        for (; t >= 0; --t) { last = s_delta[t] + gl * (s_nnt[t] * last); s_delta[t] = last + s_v[t]; }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += GAE_LONG_THREADS) returns[(size_t)t * E + e] = s_delta[t];
}

// the [T,E] table of terminal values: zeroed by a kernel on the stream (the library's rule: no memset command between its launches), then
// the K values of the batched value pass scattered to their rollout rows, one lane per k.  idx[k] = t * E + e, checked on the host when the
// row was marked (in range, no row twice); the guard below only keeps a corrupted index from leaving the table.
__global__ void fill_zero_kernel(float* p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0.f;
}
__global__ void tval_scatter_kernel(const float* val, const int* idx, int K, int n, float* tval) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int i = idx[k];
    if (i >= 0 && i < n) tval[i] = val[k];
}
