// The optimiser passes for gfx950, every opt_* entry point of include/nerfsig.h: torch.optim.Adam's update (adam.h) of the D selected codebook tables from their one
// shared gradient (opt_codebook_adam[_sel[_next[_dense]]]) and of any list of dense tensors in launch groups of kAdamGroup (opt_adam_dense[_host]); torch_ema's moving average
// of the parameters (opt_ema_update).  The scatter owners' fused form of the update, hg_levels_scatter_adam, stays in hashgrid.hip and borrows adam_prepare_launch.
#include "adam.h"

namespace nsig {

// ----------------------------------------------------------------------------- dense multi-tensor Adam (the decoder's parameters, stage 1's tables and MLPs)

// torch's fused multi-tensor Adam walks 64K-element chunks, one workgroup each: the decoder's 29 tensors (262k parameters) become
// ~30 workgroups that each stream 64K elements serially (28 us).  Here a chunk is 1024 elements, so the same update is ~260
// workgroups of one pass (~3 us).
constexpr uint32_t kDenseChunk = 1024;
struct DenseAdam {
    float *p[kAdamGroup], *m[kAdamGroup], *v[kAdamGroup], *step[kAdamGroup];
    const float *g[kAdamGroup];
    uint32_t numel[kAdamGroup], chunk0[kAdamGroup + 1];   // chunk0: first chunk of tensor i (chunk_owner)
    uint8_t slot[kAdamGroup];                             // where the tensor's two step scalars sit in the scratch (k_adam_dense_prepare's index)
};

__global__ void k_adam_dense_prepare(DenseAdam a, uint32_t n, const float *__restrict__ lr, float beta1, float beta2, float *__restrict__ scratch) {
    const uint32_t i = threadIdx.x;
    if (i >= n) return;
    const float step = *a.step[i] + 1.0f;
    *a.step[i] = step;
    adam_step_scalars(step, lr, beta1, beta2, scratch, i, kAdamGroup);
}

// chunk `chunk` (1024 elements) of tensor i, element by element; scalars(i, ss, ib): the two step scalars of tensor i, wherever the launch keeps them
template <typename Scalars>
__device__ __forceinline__ void adam_dense_chunk(const DenseAdam &a, uint32_t i, uint32_t chunk, Scalars scalars, float beta1, float beta2, float eps, float grad_scale) {
    const uint32_t base = chunk * kDenseChunk;
    float ss, ib;
    scalars(i, ss, ib);
    float *__restrict__ pp = a.p[i], *__restrict__ pm = a.m[i], *__restrict__ pv = a.v[i];
    const float *__restrict__ pg = a.g[i];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t e = base + u * 256 + threadIdx.x;
        if (e < a.numel[i]) {
            float p = pp[e], m = pm[e], v = pv[e];
            adam_update(pg[e] * grad_scale, p, m, v, beta1, beta2, eps, ss, ib);
            pp[e] = p; pm[e] = m; pv[e] = v;
        }
    }
}

__global__ void __launch_bounds__(256) k_adam_dense(DenseAdam a, uint32_t n, const float *__restrict__ scratch, float beta1, float beta2, float eps,
                                                    float grad_scale) {
    const uint32_t i = chunk_owner(a.chunk0, n);
    adam_dense_chunk(a, i, blockIdx.x - a.chunk0[i], [&](uint32_t i, float &ss, float &ib) { ss = scratch[a.slot[i]], ib = scratch[kAdamGroup + a.slot[i]]; }, beta1, beta2, eps, grad_scale);
}

// The same update with the per-tensor step size lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t) computed by the HOST (torch.optim.Adam's non-capturable state
// keeps its step counts in host tensors: opt_adam_dense_host, the drop-in model's optimiser hook).
struct DenseScalars {
    float ss[kAdamGroup], ib[kAdamGroup];
};
__global__ void __launch_bounds__(256) k_adam_dense_host(DenseAdam a, uint32_t n, DenseScalars sc, float beta1, float beta2, float eps, float grad_scale) {
    const uint32_t i = chunk_owner(a.chunk0, n);
    adam_dense_chunk(a, i, blockIdx.x - a.chunk0[i], [&](uint32_t i, float &ss, float &ib) { ss = sc.ss[i], ib = sc.ib[i]; }, beta1, beta2, eps, grad_scale);
}

// Large tensors (stage 1: sixteen 4 MiB base tables with their own gradients): 4096-element chunks, float4 per lane, sixteen 16-byte loads in
// flight per lane before the first dependent store, non-temporal loads and moment stores (a 448 MiB stream that nothing re-reads before it is evicted anyway).
constexpr uint32_t kDenseChunk4 = 4096, kDenseBigNumel = 1u << 16, kDenseRideAlong = 1024;
__device__ __forceinline__ void adam_dense_chunk4(const DenseAdam &a, uint32_t i, uint32_t chunk, float ss, float ib, float beta1, float beta2, float eps, float grad_scale) {
    const uint32_t base = chunk * (kDenseChunk4 / 4), n4 = a.numel[i] / 4;
    float4 *__restrict__ pp = reinterpret_cast<float4 *>(a.p[i]), *__restrict__ pm = reinterpret_cast<float4 *>(a.m[i]), *__restrict__ pv = reinterpret_cast<float4 *>(a.v[i]);
    const float4 *__restrict__ pg = reinterpret_cast<const float4 *>(a.g[i]);
    float4 p[4], m[4], v[4], g[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t e = min(base + u * 256u + threadIdx.x, n4 - 1u);      // clamped: the duplicate is not stored
        p[u] = ld4<true>(pp + e); m[u] = ld4<true>(pm + e); v[u] = ld4<true>(pv + e); g[u] = ld4<true>(pg + e);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t e = base + u * 256u + threadIdx.x;
        if (e >= n4) break;
        adam_update4(g[u], p[u], m[u], v[u], beta1, beta2, eps, ss, ib, grad_scale);
        // the moments stream out; the PARAMETERS go through the caches: the next step's encoder gathers from these 64 MiB (same box, two rounds: encoder 139-141 -> 129-131 us,
        // this pass 95 -> 91, step -0.6 %, on the sparse grid -1.8 %)
        st4<false>(pp + e, p[u]); st4<true>(pm + e, m[u]); st4<true>(pv + e, v[u]);
    }
}

__global__ void __launch_bounds__(256) k_adam_dense_v4(DenseAdam a, uint32_t n, const float *__restrict__ scratch, float beta1, float beta2, float eps,
                                                       float grad_scale) {
    const uint32_t i = chunk_owner(a.chunk0, n);
    adam_dense_chunk4(a, i, blockIdx.x - a.chunk0[i], scratch[a.slot[i]], scratch[kAdamGroup + a.slot[i]], beta1, beta2, eps, grad_scale);
}

// The decoder's pass as the closing workgroups of the codebook launch (k_codebook_adam_sel<.., DENSE>): one chunk table for both forms -- bit i of `wide`: tensor i
// goes in 4096-element float4 chunks (adam_dense_chunk4), else in 1024-element ones -- and the two scalars of tensor i at scratch[i], scratch[kAdamGroup + i].
// The codebook launch's 384 table addresses fill 3 KiB of the 4 KiB a launch's arguments may take, so this table travels through memory: k_adam_prepare, which
// takes it as an argument, leaves it in the launch's dense scratch (NSIG_ADAM_DENSE_SCRATCH_BYTES: the 2 * kAdamGroup scalars, then the table).
struct DenseFused {
    DenseAdam a;
    uint32_t n, wide;
};
constexpr size_t kDenseFusedTable = 2 * kAdamGroup * sizeof(float);      // the table's byte offset in the scratch
static_assert(NSIG_MAX_MESSAGE_DIM % kWave == 0 && kAdamGroup <= 32 && kDenseFusedTable % 16 == 0 && kDenseFusedTable + sizeof(DenseFused) <= NSIG_ADAM_DENSE_SCRATCH_BYTES, "dense scratch layout");

__device__ __forceinline__ void adam_dense_fused(const DenseFused &d, uint32_t block, const float *__restrict__ scratch, float beta1, float beta2, float eps, float grad_scale) {
    const uint32_t i = chunk_owner(d.a.chunk0, d.n, block), chunk = block - d.a.chunk0[i];
    if ((d.wide >> i) & 1u) adam_dense_chunk4(d.a, i, chunk, scratch[i], scratch[kAdamGroup + i], beta1, beta2, eps, grad_scale);
    else adam_dense_chunk(d.a, i, chunk, [&](uint32_t i, float &ss, float &ib) { ss = scratch[i], ib = scratch[kAdamGroup + i]; }, beta1, beta2, eps, grad_scale);
}

// ----------------------------------------------------------------------------- the codebook tables (shared gradient)

// Fused Adam over the D selected tables (shared gradient): float4 per lane, D x (param, exp_avg, exp_avg_sq) streams.
struct AdamPtrs {
    float *p[NSIG_MAX_MESSAGE_DIM];
    float *m[NSIG_MAX_MESSAGE_DIM];
    float *v[NSIG_MAX_MESSAGE_DIM];
    float step_size[NSIG_MAX_MESSAGE_DIM];
    float inv_bc2_sqrt[NSIG_MAX_MESSAGE_DIM];
};

__global__ void __launch_bounds__(256) k_codebook_adam(const float4 *__restrict__ G, AdamPtrs a, uint32_t D, float beta1, float beta2, float eps,
                                                       float grad_scale) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= NSIG_TABLE_ROWS / 2) return;
    float4 g = G[e];
    g.x *= grad_scale; g.y *= grad_scale; g.z *= grad_scale; g.w *= grad_scale;
    for (uint32_t i = 0; i < D; ++i) {
        float4 *pp = reinterpret_cast<float4 *>(a.p[i]) + e, *pm = reinterpret_cast<float4 *>(a.m[i]) + e, *pv = reinterpret_cast<float4 *>(a.v[i]) + e;
        float4 p = *pp, m = *pm, v = *pv;
        adam_update4(g, p, m, v, beta1, beta2, eps, a.step_size[i], a.inv_bc2_sqrt[i]);
        *pp = p; *pm = m; *pv = v;
    }
}

// device-side table selection (every launch argument independent of the message: the enclosing step can be captured in a hipGraph)
struct AdamPairPtrs {
    float *p[2 * NSIG_MAX_MESSAGE_DIM];
    float *m[2 * NSIG_MAX_MESSAGE_DIM];
    float *v[2 * NSIG_MAX_MESSAGE_DIM];
};
struct StepPtrs {
    float *s[2 * NSIG_MAX_MESSAGE_DIM];
};

// one thread per bit: advance the selected table's step count and derive its bias-correction scalars.  With a dense part (k_codebook_adam_sel<.., DENSE>) the launch
// has a second wave, whose thread j does the same for dense tensor j -- what k_adam_dense_prepare does in front of k_adam_dense -- and leaves the tensor's row of the
// chunk table in memory
__global__ void k_adam_prepare(StepPtrs steps, const float *__restrict__ message, uint32_t D, const float *__restrict__ lr, float beta1, float beta2,
                               float *__restrict__ scratch, DenseFused dense, DenseFused *__restrict__ dense_dev, float *__restrict__ dense_scratch) {
    uint32_t i = threadIdx.x, stride = D;
    float *sp;
    if (i < NSIG_MAX_MESSAGE_DIM) {
        if (i >= D) return;
        sp = steps.s[2 * i + (message[i] != 0.0f)];
    } else {
        i -= NSIG_MAX_MESSAGE_DIM;
        if (i >= dense.n) return;
        sp = dense.a.step[i];
        scratch = dense_scratch, stride = kAdamGroup;
        DenseAdam &t = dense_dev->a;
        t.p[i] = dense.a.p[i]; t.m[i] = dense.a.m[i]; t.v[i] = dense.a.v[i]; t.g[i] = dense.a.g[i]; t.step[i] = sp;
        t.numel[i] = dense.a.numel[i]; t.chunk0[i + 1] = dense.a.chunk0[i + 1]; t.slot[i] = (uint8_t)i;
        if (i == 0) t.chunk0[0] = 0, dense_dev->n = dense.n, dense_dev->wide = dense.wide;
    }
    const float step = *sp + 1.0f;
    *sp = step;
    adam_step_scalars(step, lr, beta1, beta2, scratch, i, stride);
}

// NEXT: the same pass also produces the pre-summed codebook of the NEXT step's message, S_next = sum_i table[2i + next_i]: where the
// next bit equals the current one the freshly updated row is already in registers, otherwise the partner table's row is read
// (about D/2 extra 4 MiB streams: +9 % traffic) -- instead of a separate 128 MiB pre-sum pass at the head of the next step.
// The sum keeps the table order, so S_next is bit-identical to k_codebook_presum_sel's.
//
// The step's selection is resolved ONCE per wave, not per table: lane i reads message[i] / next_message[i] / the two scalars of table i, two ballots make the masks
// `sel` (bit i: message[i] != 0) and `oth` (bit i: the next bit differs, S_next takes the partner's row), and the scalars of table i come out of lane i by v_readlane.
// The table loop then carries no scalar-memory dependency but the tables' addresses (kernel arguments at a computed index), and those are fetched four tables ahead.
// Four tables per trip, as a rolling pipeline over four register slots: table i is updated and stored from slot i % 4, and table i + 4 is requested into that slot
// right there -- in front of the wait for table i + 1, which vmcnt counts in issue order and so does not cover table i's stores.  A wave then keeps the rows of
// 3-4 tables in flight for the whole walk, where two tables per trip had 6-8 requests for part of a trip and nothing across the trip's stores.
//
// kSelCols = 2 columns per thread (half a table apart), so 512 workgroups of 256 threads: 8 waves per CU, 18-32 16-byte requests per thread.  The old grid's 1024
// workgroups were 16 waves per CU -- one residency wave when alone, but in the step the march-ahead's k_march_index (one wave per ray: 18 per CU) is already there and
// the two do not fit into a CU's 32 wave slots together: the workgroups that had to wait for a slot walked their 32 tables late and were the launch's tail
// (LABNOTES, "Codebook Adam beside the march-ahead").  Half the waves at twice the depth are all resident from the start and stream just as fast.
constexpr uint32_t kSelCols = 2, kSelColumns = NSIG_TABLE_ROWS / 2 / kSelCols, kSelColStride = kSelColumns * (uint32_t)sizeof(float4), kSelWalkers = kSelColumns / 256;
template <bool NEXT, bool NT, int C>
struct AdamSlot {
    float *bp, *bm, *bv;      // the selected table and its moments (wave-uniform)
    float4 p[C], m[C], v[C], o[C];      // per column; o: the partner table's row
    bool other;               // S_next takes the partner's row (wave-uniform)

    static __device__ __forceinline__ float4 *at(const float *base, uint32_t byte_off) {
        return reinterpret_cast<float4 *>(reinterpret_cast<char *>(const_cast<float *>(base)) + byte_off);
    }
    __device__ __forceinline__ void request(const AdamPairPtrs &a, uint32_t i, uint64_t sel, uint64_t oth, uint32_t byte_off) {
        const uint32_t j = 2 * i + ((uint32_t)(sel >> i) & 1u);
        bp = a.p[j]; bm = a.m[j]; bv = a.v[j];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            p[c] = ld4<NT>(at(bp, byte_off + c * kSelColStride)); m[c] = ld4<NT>(at(bm, byte_off + c * kSelColStride)); v[c] = ld4<NT>(at(bv, byte_off + c * kSelColStride));
        }
        other = NEXT && ((uint32_t)(oth >> i) & 1u);
        if (other) {
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = ld4<NT>(at(a.p[j ^ 1u], byte_off + c * kSelColStride));
        }
        __builtin_amdgcn_sched_barrier(0);      // the requests stay here, in front of the next table's update (LABNOTES 17a: the scheduler moves them to their first use)
    }
    // torch's update of table i, its stores, and S_next's term of the table: the fresh row or the partner's
    __device__ __forceinline__ void update_store(const float4 *g, uint32_t i, float sc_ss, float sc_ib, float beta1, float beta2, float eps, uint32_t byte_off, float4 *acc) {
        const float ss = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sc_ss), (int)i));
        const float ib = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sc_ib), (int)i));
#pragma unroll
        for (int c = 0; c < C; ++c) {
            adam_update4(g[c], p[c], m[c], v[c], beta1, beta2, eps, ss, ib);
            st4<NT>(at(bp, byte_off + c * kSelColStride), p[c]); st4<NT>(at(bm, byte_off + c * kSelColStride), m[c]); st4<NT>(at(bv, byte_off + c * kSelColStride), v[c]);
            if (NEXT) {
                const float4 t = other ? o[c] : p[c];
                acc[c].x += t.x; acc[c].y += t.y; acc[c].z += t.z; acc[c].w += t.w;
                // the sum is taken HERE: left alone, the compiler sinks the four tables' adds to the end of the trip, keeps every o alive until then, loads the next
                // partner rows into other registers and copies them over behind a vmcnt(0) -- a full drain of the trip's loads and stores
                asm volatile("" : "+v"(acc[c].x), "+v"(acc[c].y), "+v"(acc[c].z), "+v"(acc[c].w));
            }
        }
    }
};

//
// DENSE: the launch closes with the workgroups of the dense chunk table, which step the decoder's tensors (adam_dense_fused) behind the 512 that walk the tables: the branch is
// uniform per workgroup, at the kernel's top, and the walk keeps its index.  The decoder's update needs nothing of the walk and the walk nothing of it; as a launch of
// its own (with its prepare launch) it stood behind the walk, at the end of the step.  BEHIND the walkers, not in front of them: the walkers fill every wave slot
// this kernel's registers leave (two workgroups per CU), so workgroups ahead of them in the grid hold 260 of those slots when the walk starts and that many walkers
// start late -- measured, the step lost what the two launches had cost and more (LABNOTES, "Optimiser tail").  At the grid's end they take the slots of the first
// walkers to finish, while the last are still streaming.
template <bool NEXT, bool NT, bool DENSE = false>
__global__ void __launch_bounds__(256) k_codebook_adam_sel(const float4 *__restrict__ G, AdamPairPtrs a, const float *__restrict__ message,
                                                           const float *__restrict__ scratch, uint32_t D, float beta1, float beta2, float eps,
                                                           float grad_scale, const float *__restrict__ next_message, float4 *__restrict__ S_next,
                                                           const DenseFused *__restrict__ dense = nullptr,
                                                           const float *__restrict__ dense_scratch = nullptr, float dense_grad_scale = 1.0f) {
    constexpr int C = kSelCols;
    if (DENSE && blockIdx.x >= kSelWalkers) {
        adam_dense_fused(*dense, blockIdx.x - kSelWalkers, dense_scratch, beta1, beta2, eps, dense_grad_scale);
        return;
    }
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= kSelColumns) return;      // (whole waves: the grid is a multiple of 256)
    const uint32_t lane = threadIdx.x & 63u, byte_off = e * (uint32_t)sizeof(float4);
    const bool bit = lane < D && message[lane] != 0.0f;
    const uint64_t sel = __ballot(bit);
    const uint64_t oth = NEXT ? __ballot(lane < D && (next_message[lane] != 0.0f) != bit) : 0;
    const float sc_ss = lane < D ? scratch[lane] : 0.f, sc_ib = lane < D ? scratch[D + lane] : 0.f;      // D <= NSIG_MAX_MESSAGE_DIM = one wave's lanes
    float4 g[C], acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        g[c] = ld4<NT>(G + e + c * kSelColumns);
        g[c].x *= grad_scale; g[c].y *= grad_scale; g[c].z *= grad_scale; g[c].w *= grad_scale;
        acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    AdamSlot<NEXT, NT, C> slot[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        if (k < D) slot[k].request(a, k, sel, oth, byte_off);
    uint32_t i = 0;
    for (; i + 8 <= D; i += 4) {      // every table of the trip has a successor four tables on
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            slot[k].update_store(g, i + k, sc_ss, sc_ib, beta1, beta2, eps, byte_off, acc);
            slot[k].request(a, i + k + 4, sel, oth, byte_off);
        }
    }
    for (; i < D; i += 4) {           // the last 1 .. 7 tables: D % 4 and D < 4 (a rank's share of the sharded optimiser) end here
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (i + k >= D) break;
            slot[k].update_store(g, i + k, sc_ss, sc_ib, beta1, beta2, eps, byte_off, acc);
            if (i + k + 4 < D) slot[k].request(a, i + k + 4, sel, oth, byte_off);
        }
    }
    if (NEXT) {
#pragma unroll
        for (int c = 0; c < C; ++c) S_next[e + c * kSelColumns] = acc[c];
    }
}

// ----------------------------------------------------------------------------- EMA of the parameters
// The stage-1 trainer keeps an exponential moving average of every parameter (main_nerf.py:130 `ema_decay=0.95`; utils.py:389-390 torch_ema's
// ExponentialMovingAverage, updated after every optimiser step, :761-762/:892-893) and evaluates / checkpoints with it (:801-811).  torch_ema 0.3's update(), with
// its default warm-up (use_num_updates): num_updates += 1; decay = min(decay, (1 + num_updates) / (10 + num_updates)); then for every parameter
//     tmp = shadow - param;  tmp *= (1 - decay);  shadow -= tmp
// -- here one launch over all tensors, the update count read from the captured loop's device step counter (which the step's loss kernel has already advanced).
constexpr int kEmaMax = 32;
constexpr uint32_t kEmaChunk = 4096;      // elements per workgroup
struct DenseEma {
    const float *p[kEmaMax];
    float *s[kEmaMax];
    uint32_t numel[kEmaMax], chunk0[kEmaMax + 1];
};
__global__ void __launch_bounds__(256) k_ema_dense(DenseEma a, uint32_t n, const uint32_t *__restrict__ num_updates, double decay) {
    const uint32_t t = chunk_owner(a.chunk0, n);
    const double nu = (double)*num_updates;
    const float w = (float)(1.0 - fmin(decay, (1.0 + nu) / (10.0 + nu)));      // (python: a double, handed to mul_ as a float32 scalar)
    const uint32_t first = (blockIdx.x - a.chunk0[t]) * kEmaChunk, numel = a.numel[t];
    const float *__restrict__ p = a.p[t];
    float *__restrict__ s = a.s[t];
    if (numel % 4u == 0 && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(s)) & 15) == 0) {      // (uniform)
        for (uint32_t i = first + 4u * threadIdx.x; i < min(numel, first + kEmaChunk); i += 1024u) {
            const float4 pv = *reinterpret_cast<const float4 *>(p + i);
            float4 sv = *reinterpret_cast<const float4 *>(s + i);
            sv.x = sv.x - (sv.x - pv.x) * w; sv.y = sv.y - (sv.y - pv.y) * w; sv.z = sv.z - (sv.z - pv.z) * w; sv.w = sv.w - (sv.w - pv.w) * w;
            *reinterpret_cast<float4 *>(s + i) = sv;
        }
    } else {
        for (uint32_t i = first + threadIdx.x; i < min(numel, first + kEmaChunk); i += 256u) s[i] = s[i] - (s[i] - p[i]) * w;
    }
}

}  // namespace nsig

using namespace nsig;

// Tensor k (numel elements, `chunk` per workgroup) joins a launch's chunk table: chunk0[k] its first workgroup, chunk0[k + 1] the grid so far (the structs start zeroed)
static void chunk_table_append(uint32_t *numel_tab, uint32_t *chunk0, uint32_t k, uint32_t numel, uint32_t chunk) {
    numel_tab[k] = numel;
    chunk0[k + 1] = chunk0[k] + ceil_div(numel, chunk);
}

static const char *const kNullTable = "%s: table %u has a null pointer", *const kMisalignedTable = "%s: table %u is not 16-byte aligned";

NSIG_EXPORT int opt_codebook_adam(const float *G, float *const *params_host, float *const *exp_avg_host, float *const *exp_avg_sq_host,
                                  uint32_t D, float beta1, float beta2, float eps, const float *step_size_host,
                                  const float *inv_bc2_sqrt_host, float grad_scale, nsig_stream_t stream) {
    NSIG_REQUIRE(G && params_host && exp_avg_host && exp_avg_sq_host && step_size_host && inv_bc2_sqrt_host, "opt_codebook_adam: null pointer");
    NSIG_REQUIRE(D >= 1 && D <= NSIG_MAX_MESSAGE_DIM, "opt_codebook_adam: D=%u out of range", D);
    NSIG_REQUIRE(aligned16(G), "opt_codebook_adam: G must be 16-byte aligned");
    AdamPtrs a{};
    if (int e = take_pointers({a.p, a.m, a.v}, {params_host, exp_avg_host, exp_avg_sq_host}, D, "opt_codebook_adam", kNullTable, kMisalignedTable)) return e;
    for (uint32_t i = 0; i < D; ++i) {
        a.step_size[i] = step_size_host[i];
        a.inv_bc2_sqrt[i] = inv_bc2_sqrt_host[i];
    }
    k_codebook_adam<<<NSIG_TABLE_ROWS / 2 / 256, 256, 0, as_stream(stream)>>>(reinterpret_cast<const float4 *>(G), a, D, beta1, beta2, eps, grad_scale);
    return check_launch("opt_codebook_adam");
}

// Which of a group's tensors take the wide form (bit i: tensor first + i).  A group with a large tensor launches the wide kernel anyway: its medium-sized tensors
// (stage 1: the two MLPs' 3072 + 7168 parameters beside sixteen 4 MiB tables) ride along as a few more workgroups instead of a launch of their own on the step's
// serial tail (the same update, element by element)
static uint32_t wide_tensors(uint32_t cnt, float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq, const uint32_t *numel) {
    auto vectorisable = [&](uint32_t j) { return numel[j] % 4 == 0 && aligned16(params[j]) && aligned16(grads[j]) && aligned16(exp_avg[j]) && aligned16(exp_avg_sq[j]); };
    bool any_big = false;
    for (uint32_t j = 0; j < cnt; ++j) any_big = any_big || (numel[j] >= kDenseBigNumel && vectorisable(j));
    uint32_t wide = 0;
    for (uint32_t j = 0; j < cnt; ++j) wide |= (uint32_t)(numel[j] >= (any_big ? kDenseRideAlong : kDenseBigNumel) && vectorisable(j)) << j;
    return wide;
}

static const char *const kNullTensor = "%s: tensor %u has a null pointer or no elements";

// dense: the decoder's part of opt_codebook_adam_sel_next_dense (n == 0: none); dense_scratch: NSIG_ADAM_DENSE_SCRATCH_BYTES
static int codebook_adam_sel(const char *who, const float *G, float *const *params_host, float *const *exp_avg_host, float *const *exp_avg_sq_host,
                             float *const *steps_host, const float *message, uint32_t D, const float *lr, float beta1, float beta2,
                             float eps, float grad_scale, float *scratch, const float *next_message, float *S_next, nsig_stream_t stream,
                             const DenseFused &dense = DenseFused{}, void *dense_scratch = nullptr, float dense_grad_scale = 1.0f) {
    NSIG_REQUIRE(G && params_host && exp_avg_host && exp_avg_sq_host && steps_host && message && lr && scratch, "%s: null pointer", who);
    NSIG_REQUIRE(D >= 1 && D <= NSIG_MAX_MESSAGE_DIM, "%s: D=%u out of range", who, D);
    NSIG_REQUIRE(aligned16(G), "%s: G must be 16-byte aligned", who);
    AdamPairPtrs a{};
    StepPtrs s{};
    if (int e = take_pointers({a.p, a.m, a.v, s.s}, {params_host, exp_avg_host, exp_avg_sq_host, steps_host}, 2 * D, who, kNullTable, kMisalignedTable, 3)) return e;
    hipStream_t st = as_stream(stream);
    float *dense_scalars = reinterpret_cast<float *>(dense_scratch);
    DenseFused *dense_dev = dense.n ? reinterpret_cast<DenseFused *>(reinterpret_cast<char *>(dense_scratch) + kDenseFusedTable) : nullptr;
    k_adam_prepare<<<1, NSIG_MAX_MESSAGE_DIM + (dense.n ? kAdamGroup : 0), 0, st>>>(s, message, D, lr, beta1, beta2, scratch, dense, dense_dev, dense_scalars);
    if (int e = check_launch(who)) return e;
    const float4 *G4 = reinterpret_cast<const float4 *>(G);
    float4 *S4 = reinterpret_cast<float4 *>(S_next);
    const uint32_t walk = kSelWalkers, dense_chunks = dense.a.chunk0[dense.n];
    // non-temporal accesses (same-box A/B of the bench step, three pairs: 1.124-1.138 ms against 1.151-1.157 with plain accesses; the kernel alone takes
    // the same 160-164 us either way, the next step's gather gains)
    if (dense.n && next_message)
        k_codebook_adam_sel<true, true, true><<<dense_chunks + walk, 256, 0, st>>>(G4, a, message, scratch, D, beta1, beta2, eps, grad_scale, next_message, S4,
                                                                                   dense_dev, dense_scalars, dense_grad_scale);
    else if (dense.n)
        k_codebook_adam_sel<false, false, true><<<dense_chunks + walk, 256, 0, st>>>(G4, a, message, scratch, D, beta1, beta2, eps, grad_scale, nullptr, nullptr,
                                                                                     dense_dev, dense_scalars, dense_grad_scale);
    else if (next_message)
        k_codebook_adam_sel<true, true><<<walk, 256, 0, st>>>(G4, a, message, scratch, D, beta1, beta2, eps, grad_scale, next_message, S4);
    else
        k_codebook_adam_sel<false, false><<<walk, 256, 0, st>>>(G4, a, message, scratch, D, beta1, beta2, eps, grad_scale, nullptr, nullptr);
    return check_launch(who);
}

NSIG_EXPORT int opt_codebook_adam_sel(const float *G, float *const *params_host, float *const *exp_avg_host, float *const *exp_avg_sq_host,
                                      float *const *steps_host, const float *message, uint32_t D, const float *lr, float beta1, float beta2,
                                      float eps, float grad_scale, float *scratch, nsig_stream_t stream) {
    return codebook_adam_sel("opt_codebook_adam_sel", G, params_host, exp_avg_host, exp_avg_sq_host, steps_host, message, D, lr, beta1, beta2, eps,
                             grad_scale, scratch, nullptr, nullptr, stream);
}

NSIG_EXPORT int opt_codebook_adam_sel_next(const float *G, float *const *params_host, float *const *exp_avg_host, float *const *exp_avg_sq_host,
                                           float *const *steps_host, const float *message, uint32_t D, const float *lr, float beta1, float beta2,
                                           float eps, float grad_scale, float *scratch, const float *next_message, float *S_next,
                                           nsig_stream_t stream) {
    NSIG_REQUIRE(next_message && S_next && aligned16(S_next), "opt_codebook_adam_sel_next: next_message / S_next null or S_next not 16-byte aligned");
    return codebook_adam_sel("opt_codebook_adam_sel_next", G, params_host, exp_avg_host, exp_avg_sq_host, steps_host, message, D, lr, beta1, beta2, eps,
                             grad_scale, scratch, next_message, S_next, stream);
}

NSIG_EXPORT int opt_codebook_adam_sel_next_dense(const float *G, float *const *params_host, float *const *exp_avg_host, float *const *exp_avg_sq_host,
                                                 float *const *steps_host, const float *message, uint32_t D, const float *lr, float beta1, float beta2,
                                                 float eps, float grad_scale, float *scratch, const float *next_message, float *S_next, uint32_t n_dense,
                                                 float *const *dense_params_host, const float *const *dense_grads_host, float *const *dense_exp_avg_host,
                                                 float *const *dense_exp_avg_sq_host, float *const *dense_steps_host, const uint32_t *dense_numel_host,
                                                 float dense_grad_scale, void *dense_scratch, nsig_stream_t stream) {
    const char *who = "opt_codebook_adam_sel_next_dense";
    NSIG_REQUIRE((next_message == nullptr) == (S_next == nullptr) && aligned16(S_next), "%s: next_message / S_next go together and S_next is 16-byte aligned", who);
    NSIG_REQUIRE(n_dense <= (uint32_t)kAdamGroup, "%s: at most %d dense tensors ride in the launch", who, kAdamGroup);
    DenseFused dense{};
    if (n_dense) {
        NSIG_REQUIRE(dense_params_host && dense_grads_host && dense_exp_avg_host && dense_exp_avg_sq_host && dense_steps_host && dense_numel_host && dense_scratch,
                     "%s: null pointer", who);
        NSIG_REQUIRE(aligned16(dense_scratch), "%s: dense_scratch must be 16-byte aligned", who);
        for (uint32_t i = 0; i < n_dense; ++i) NSIG_REQUIRE(dense_numel_host[i] > 0, kNullTensor, who, i);
        if (int e = take_pointers({dense.a.p, dense.a.m, dense.a.v, dense.a.step}, {dense_params_host, dense_exp_avg_host, dense_exp_avg_sq_host, dense_steps_host}, n_dense,
                                  who, kNullTensor))
            return e;
        if (int e = take_pointers({dense.a.g}, {dense_grads_host}, n_dense, who, kNullTensor)) return e;
        dense.n = n_dense;
        dense.wide = wide_tensors(n_dense, dense_params_host, dense_grads_host, dense_exp_avg_host, dense_exp_avg_sq_host, dense_numel_host);
        for (uint32_t i = 0; i < n_dense; ++i) chunk_table_append(dense.a.numel, dense.a.chunk0, i, dense_numel_host[i], (dense.wide >> i) & 1u ? kDenseChunk4 : kDenseChunk);
    }
    return codebook_adam_sel(who, G, params_host, exp_avg_host, exp_avg_sq_host, steps_host, message, D, lr, beta1, beta2, eps, grad_scale, scratch, next_message,
                             S_next, stream, dense, dense_scratch, dense_grad_scale);
}

int nsig::adam_prepare_launch(float *const *steps_host, uint32_t n, const float *lr, float beta1, float beta2, float *scratch, hipStream_t st, const char *who) {
    DenseAdam all{};
    for (uint32_t i = 0; i < n; ++i) all.step[i] = steps_host[i];
    k_adam_dense_prepare<<<1, kAdamGroup, 0, st>>>(all, n, lr, beta1, beta2, scratch);
    return check_launch(who);
}

NSIG_EXPORT int opt_adam_dense_host(uint32_t n, float *const *params_host, const float *const *grads_host, float *const *exp_avg_host,
                                    float *const *exp_avg_sq_host, const uint32_t *numel_host, const float *step_sizes_host, const float *inv_bc2_host,
                                    float beta1, float beta2, float eps, float grad_scale, nsig_stream_t stream) {
    NSIG_REQUIRE(params_host && grads_host && exp_avg_host && exp_avg_sq_host && numel_host && step_sizes_host && inv_bc2_host, "opt_adam_dense_host: null pointer");
    hipStream_t st = as_stream(stream);
    for (uint32_t first = 0; first < n; first += kAdamGroup) {
        const uint32_t cnt = n - first < (uint32_t)kAdamGroup ? n - first : (uint32_t)kAdamGroup;
        DenseAdam a{};
        DenseScalars sc{};
        for (uint32_t i = 0; i < cnt; ++i) {
            const uint32_t j = first + i;
            NSIG_REQUIRE(params_host[j] && grads_host[j] && exp_avg_host[j] && exp_avg_sq_host[j] && numel_host[j] > 0,
                         "opt_adam_dense_host: tensor %u has a null pointer or no elements", j);
            a.p[i] = params_host[j]; a.g[i] = grads_host[j]; a.m[i] = exp_avg_host[j]; a.v[i] = exp_avg_sq_host[j];
            chunk_table_append(a.numel, a.chunk0, i, numel_host[j], kDenseChunk);
            sc.ss[i] = step_sizes_host[j];
            sc.ib[i] = inv_bc2_host[j];
        }
        k_adam_dense_host<<<a.chunk0[cnt], 256, 0, st>>>(a, cnt, sc, beta1, beta2, eps, grad_scale);
        if (int e = check_launch("opt_adam_dense_host")) return e;
    }
    return NSIG_OK;
}

NSIG_EXPORT int opt_adam_dense(uint32_t n, float *const *params_host, const float *const *grads_host, float *const *exp_avg_host,
                               float *const *exp_avg_sq_host, float *const *steps_host, const uint32_t *numel_host, const float *lr, float beta1,
                               float beta2, float eps, float grad_scale, float *scratch, nsig_stream_t stream) {
    NSIG_REQUIRE(params_host && grads_host && exp_avg_host && exp_avg_sq_host && steps_host && numel_host && lr && scratch, "opt_adam_dense: null pointer");
    hipStream_t st = as_stream(stream);
    for (uint32_t first = 0; first < n; first += kAdamGroup) {   // 32 tensors per group of launches
        const uint32_t cnt = n - first < (uint32_t)kAdamGroup ? n - first : (uint32_t)kAdamGroup;
        DenseAdam small{}, big{};
        uint32_t n_small = 0, n_big = 0;
        const uint32_t wide_mask = wide_tensors(cnt, params_host + first, grads_host + first, exp_avg_host + first, exp_avg_sq_host + first, numel_host + first);
        for (uint32_t i = 0; i < cnt; ++i) {
            const uint32_t j = first + i;
            NSIG_REQUIRE(params_host[j] && grads_host[j] && exp_avg_host[j] && exp_avg_sq_host[j] && steps_host[j] && numel_host[j] > 0, kNullTensor, "opt_adam_dense", j);
            const bool wide = (wide_mask >> i) & 1u;
            DenseAdam &d = wide ? big : small;
            uint32_t &k = wide ? n_big : n_small;
            d.p[k] = params_host[j]; d.g[k] = grads_host[j]; d.m[k] = exp_avg_host[j]; d.v[k] = exp_avg_sq_host[j];
            d.slot[k] = (uint8_t)i;
            chunk_table_append(d.numel, d.chunk0, k, numel_host[j], wide ? kDenseChunk4 : kDenseChunk);
            ++k;
        }
        float *sc = scratch + (size_t)first * 2;
        if (int e = adam_prepare_launch(steps_host + first, cnt, lr, beta1, beta2, sc, st, "opt_adam_dense (prepare)")) return e;
        if (n_big) {
            k_adam_dense_v4<<<big.chunk0[n_big], 256, 0, st>>>(big, n_big, sc, beta1, beta2, eps, grad_scale);
            if (int e = check_launch("opt_adam_dense (wide)")) return e;
        }
        if (n_small) {
            k_adam_dense<<<small.chunk0[n_small], 256, 0, st>>>(small, n_small, sc, beta1, beta2, eps, grad_scale);
            if (int e = check_launch("opt_adam_dense")) return e;
        }
    }
    return NSIG_OK;
}

NSIG_EXPORT int opt_ema_update(uint32_t n, const float *const *params_host, float *const *shadow_host, const uint32_t *numel_host, const uint32_t *num_updates,
                               double decay, nsig_stream_t stream) {
    NSIG_REQUIRE(params_host && shadow_host && numel_host && num_updates, "opt_ema_update: null pointer");
    NSIG_REQUIRE(n >= 1 && n <= (uint32_t)kEmaMax && decay >= 0.0 && decay <= 1.0, "opt_ema_update: 1 .. %d tensors, decay in [0, 1]", kEmaMax);
    DenseEma a{};
    for (uint32_t i = 0; i < n; ++i) {
        NSIG_REQUIRE(params_host[i] && shadow_host[i] && numel_host[i] > 0, "opt_ema_update: tensor %u has a null pointer or no elements", i);
        a.p[i] = params_host[i]; a.s[i] = shadow_host[i];
        chunk_table_append(a.numel, a.chunk0, i, numel_host[i], kEmaChunk);
    }
    k_ema_dense<<<a.chunk0[n], 256, 0, as_stream(stream)>>>(a, n, num_updates, decay);
    return check_launch("opt_ema_update");
}
