// Rank-r weight gradient of a LoRA factor for gfx950:  G[f][r] = alpha * sum_{row < rows} big[row][f] * small[row][r]
// (16-bit operands, fp32 accumulation on the MFMA pipe, one rounding to the output dtype).
//
// What it replaces: peft's lora_A / lora_B are two nn.Linear modules, so under the reference's LoRA fine-tune (llava/train/train.py:873-889 -> peft ->
// torch autograd) each factor's gradient is grad_output^T @ input of a linear whose one side is r = 64 .. 256 wide:
//   dB [out][r] = dy^T u     big = dy [rows][out], small = u  = x A^T  [rows][r]
//   dA [r][in]  = du^T x     big = x  [rows][in],  small = du = dy B   [rows][r], stored transposed
// A long contraction (up to 32768 rows) with a narrow output, every operand read once.  gemm8t.hip (256 x 256 tiles, no split of the contraction) does not take
// the shape; padded to it, it would occupy 16 - 43 of 256 CUs.
//
// Here a 256-thread workgroup owns 64 columns of `big`, all R columns of `small`, and one SLICE of the rows (a whole number of 64-row K-steps).  Both operands
// stay in their forward layout: the contraction index is the slow index in memory, a K-step is staged in LDS as [row / 4][column / 16][4 rows][16 columns]
// (the image of gemm8t.hip) and the MFMA fragments come out through the gfx950 transpose read ds_read_b64_tr_b16 (tools/probes/tr_b16_probe.hip prints the lane
// mapping).  Lanes 0-31 of a read cover two adjacent 128-byte blocks = 256 contiguous bytes: conflict-free.  Staging is global -> registers -> LDS, two LDS
// buffers, the loads of K-step k + 1 issued before the products of K-step k, one barrier per K-step; every address is formed from (row < rows of the slice,
// column inside the window), so nothing outside the operands is read.
// Wave (wf, wr) of the four multiplies big columns wf * 32 .. + 31 with small columns wr * R / 2 .. + R / 2 - 1: R / 64 accumulator blocks of 32 x 32.
//
// Reduction: each workgroup writes its fp32 partial tile to workspace[slice][F][R]; a second launch sums the slices IN SLICE ORDER, applies alpha, rounds once
// and stores [F][R_out] or, transposed, [R_out][F] (columns R_out .. R - 1 are padding and are dropped).  No atomics: same inputs, same bits.
// Gradient accumulation (micro-batch i > 0 of an optimiser step): the reducer adds what `out` holds, in fp32, before that one rounding:
// out = T(alpha * sum + fp32(out)); the element is read by the thread that then stores it.
//
// LoRA dropout (dropout.h: peft's lora_A(dropout(x)), p = 0.05 in the reference's scripts).  The mask is a function of (row, column group, stream, step), so no
// masked copy of x exists anywhere: lora_wgrad_drop_kernel applies mask and scale to the big operand's chunks in registers on their way to LDS
// (dA = du^T dropout(x)), and lora_down_dropout_kernel does the same in front of the forward's u = dropout(x) A^T (below).
#include <mutex>

#include "common.h"
#include "dispatch.h"
#include "kernels.h"
#include "gemm_common.h"

namespace lmx {

namespace {

constexpr int LW_THREADS = 256;
constexpr int LW_BIG_BYTES = 64 * 64 * 2;          // one K-step of the big operand's column tile
constexpr int LW_MIN_KSTEPS = 4;                   // the automatic split leaves every slice at least this many K-steps

typedef short v4s_t __attribute__((ext_vector_type(4)));
typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s_t lds_v4s_t;

struct LoraWgradArgs {
    const void* big;
    const void* small;
    float* ws;
    int ld_big, ld_small, F, nk, S;
};
struct LoraWgradDropArgs : LoraWgradArgs {
    DropSpec d;
};

struct LoraDownArgs {
    const void* x;
    const void* A;
    void* u;
    int ldx, lda, ldu, rtiles, nk, G;
    DropSpec d;
};

constexpr int lw_lds_bytes(int NR) { return 2 * LW_BIG_BYTES * (1 + NR); }
constexpr int ld_lds_bytes(int NR) { return 2 * (64 + 64 * NR) * GEMM_ROWB; }      // two buffers of 64 x rows + 64 NR A rows, one K-step (128 bytes) each

// byte offset of the 16-byte chunk (row r of the K-step, columns 8 c8 .. + 7) in an image whose group of 4 rows takes rg bytes
__device__ __forceinline__ int lw_chunk_off(int r, int c8, int rg) { return (r >> 2) * rg + (c8 >> 1) * 128 + (r & 3) * 32 + (c8 & 1) * 16; }

// dropout of one 16-byte chunk (8 columns of a 16-bit row; bit j of `keep` = column j): kept elements scaled in fp32 and rounded once, dropped ones +0 (a
// select, not a product: a NaN under a dropped position does not pass)
template <typename T> __device__ __forceinline__ v4u_t drop_chunk16(v4u_t c, uint32_t keep, float scale) {
    v4u_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float lo = (keep >> (2 * i) & 1) ? unpack_lo<T>(c[i]) * scale : 0.f;
        const float up = (keep >> (2 * i + 1) & 1) ? unpack_hi<T>(c[i]) * scale : 0.f;
        o[i] = pack2<T>(lo, up);
    }
    return o;
}

}  // namespace

// the body of both entry points below; DROP: mask and scale (a.d) on the big operand's chunks between gload and lstore
template <typename T, int NR, bool DROP, typename Args>
__device__ __forceinline__ void lora_wgrad_tile(const Args& a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int R = 64 * NR;
    constexpr int RGB = 64 * 8, RGS = R * 8;          // bytes per group of 4 rows: big tile, small tile
    constexpr int BUF = LW_BIG_BYTES * (1 + NR);      // one K-step: big image, then small image
    constexpr int CPR = R / 8;                        // 16-byte chunks per small row

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wf = wave & 1, wr = wave >> 1;
    const int hi = lane >> 5, l31 = lane & 31;

    const int ftiles = a.F >> 6;
    const int slice = blockIdx.x / ftiles, tile = blockIdx.x - slice * ftiles;
    const int f0 = tile << 6;
    // K-steps of this slice: nk / S each, the first nk % S slices one more
    const int base = a.nk / a.S, rem = a.nk - base * a.S;
    const int kb = slice * base + (slice < rem ? slice : rem);
    const int kn = base + (slice < rem ? 1 : 0);

    const T* __restrict__ big = reinterpret_cast<const T*>(a.big);
    const T* __restrict__ small = reinterpret_cast<const T*>(a.small);

    v4u_t gb[2], gs[2 * NR];
    uint32_t keep[2];                                 // DROP: the masks of gb[], from the GLOBAL row kt * 64 + r (a slice-local row would repeat the mask per slice)
    auto gload = [&](int kt) {
        const size_t row0 = (size_t)kt * 64;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + LW_THREADS * i, r = id >> 3, c8 = id & 7;
            gb[i] = *reinterpret_cast<const v4u_t*>(big + (row0 + r) * a.ld_big + f0 + c8 * 8);
            if constexpr (DROP) keep[i] = dropout_keep8(a.d, (uint32_t)(kt * 64 + r), (uint32_t)((f0 >> 3) + c8));
        }
#pragma unroll
        for (int i = 0; i < 2 * NR; ++i) {
            const int id = tid + LW_THREADS * i, r = id / CPR, c8 = id - r * CPR;
            gs[i] = *reinterpret_cast<const v4u_t*>(small + (row0 + r) * a.ld_small + c8 * 8);
        }
    };
    auto lstore = [&](int buf) {
        char* b = smem + buf * BUF;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + LW_THREADS * i, r = id >> 3, c8 = id & 7;
            if constexpr (DROP) gb[i] = drop_chunk16<T>(gb[i], keep[i], a.d.scale);
            *reinterpret_cast<v4u_t*>(b + lw_chunk_off(r, c8, RGB)) = gb[i];
        }
#pragma unroll
        for (int i = 0; i < 2 * NR; ++i) {
            const int id = tid + LW_THREADS * i, r = id / CPR, c8 = id - r * CPR;
            *reinterpret_cast<v4u_t*>(b + LW_BIG_BYTES + lw_chunk_off(r, c8, RGS)) = gs[i];
        }
    };

    // fragment = 32 columns x 16 rows: 16-lane group g reads column block g & 1 of row block g >> 1 (8 rows = two groups of 4); lane i of the group supplies
    // row i >> 2, columns 4 (i & 3) .. + 3 and receives column i's four rows.  Every lane reads (EXEC is full: the K loop is uniform).
    __attribute__((address_space(3))) char* lds3 = (__attribute__((address_space(3))) char*)smem;
    const int i16 = lane & 15, g = lane >> 4;
    const int in_block = (g & 1) * 128 + (i16 >> 2) * 32 + (i16 & 3) * 8;
    const int boff = wf * 256 + in_block + (g >> 1) * 2 * RGB;
    const int soff = LW_BIG_BYTES + wr * NR * 256 + in_block + (g >> 1) * 2 * RGS;
    auto frag = [&](int off, int rg) -> uint4 {
        const v4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<lds_v4s_t*>(lds3 + off));
        const v4s_t up = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<lds_v4s_t*>(lds3 + off + rg));
        const uint2 l2 = __builtin_bit_cast(uint2, lo), u2 = __builtin_bit_cast(uint2, up);
        return uint4{l2.x, l2.y, u2.x, u2.y};
    };

    f32x16 acc[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

    gload(kb);
    lstore(0);
    __syncthreads();
    for (int k = 0; k < kn; ++k) {
        const int buf = k & 1;
        const bool more = k + 1 < kn;                 // uniform
        if (more) gload(kb + k + 1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const uint4 fb = frag(buf * BUF + boff + ks * 4 * RGB, RGB);
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const uint4 fs = frag(buf * BUF + soff + j * 256 + ks * 4 * RGS, RGS);
                acc[j] = Mfma32x32x16<T>::run(fs, fb, acc[j]);
            }
        }
        if (more) lstore(buf ^ 1);                    // last read in K-step k - 1, which every wave left at the barrier below
        __syncthreads();
    }

    // acc[j][4 q + e] = partial G[f0 + wf * 32 + l31][wr * R / 2 + j * 32 + 8 q + 4 hi + e]
    float* __restrict__ ws = a.ws + ((size_t)slice * a.F + f0 + wf * 32 + l31) * R + wr * (R / 2) + 4 * hi;
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<float4*>(ws + j * 32 + 8 * q) = make_float4(acc[j][4 * q], acc[j][4 * q + 1], acc[j][4 * q + 2], acc[j][4 * q + 3]);
}

template <typename T, int NR>
__global__ __launch_bounds__(LW_THREADS) void lora_wgrad_kernel(LoraWgradArgs a) { lora_wgrad_tile<T, NR, false>(a); }
template <typename T, int NR>
__global__ __launch_bounds__(LW_THREADS) void lora_wgrad_drop_kernel(LoraWgradDropArgs a) { lora_wgrad_tile<T, NR, true>(a); }

// u[m][g Rp + n] = sum_k dropout_g(x)[m][k] A[g Rp + n][k]: the forward of the G <= 3 adapters that share the input x, A = their stacked lora_A factors.  An NT
// product (both operands run along K in memory), so the tile image and the fragment reads are those of gemm.hip's register-staged kernel: a K-step of 64 is a
// 128-byte LDS row per tile row, 16-byte chunks XOR-swizzled (lds_chunk_off), ds_read_b128 fragments, weights as the MFMA's A operand.  A 256-thread workgroup
// owns 64 rows of x and ALL Rp columns of ONE adapter (wave (wm, wn): rows wm * 32 .. + 31, columns wn * Rp / 2 .. + Rp / 2 - 1 = NR accumulator blocks), so every
// chunk of x gets exactly one Philox call per adapter, made while the chunk's load is in flight; mask and scale are applied in lstore, between the registers and
// LDS.  Two LDS buffers of (64 + Rp) rows: 32 / 48 / 64 / 80 KiB for Rp = 64 .. 256, i.e. 5 / 3 / 2 / 2 workgroups per CU of the 160 KiB.
// x is read once per adapter.  The G workgroups of a row tile are blocks b, b + 8, .., which round-robin dispatch hands to the same XCD: the re-reads are MEANT to be
// L2 hits rather than HBM traffic.  That has not been checked with counters; profiles/EXPERIMENTS.md holds the timings against the materialising path.
template <typename T, int NR>
__global__ __launch_bounds__(LW_THREADS) void lora_down_dropout_kernel(LoraDownArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int Rp = 64 * NR;
    constexpr int BUF = (64 + Rp) * GEMM_ROWB;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    const int hi = lane >> 5, l31 = lane & 31;

    const int b = blockIdx.x;
    const int g = (b >> 3) % a.G;
    const int rt = (b / (8 * a.G)) * 8 + (b & 7);
    if (rt >= a.rtiles) return;                       // the grid is rounded up to 8 row tiles; uniform, before any barrier
    const int m0 = rt * 64;

    const T* __restrict__ x = reinterpret_cast<const T*>(a.x) + (size_t)m0 * a.ldx;
    const T* __restrict__ A = reinterpret_cast<const T*>(a.A) + (size_t)g * Rp * a.lda;
    DropSpec d = a.d;
    d.stream += (uint32_t)g;

    v4u_t gx[2], ga[2 * NR];
    uint32_t keep[2];
    auto gload = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + LW_THREADS * i, r = id >> 3, c8 = id & 7;
            gx[i] = *reinterpret_cast<const v4u_t*>(x + (size_t)r * a.ldx + kt * 64 + c8 * 8);
            keep[i] = dropout_keep8(d, (uint32_t)(m0 + r), (uint32_t)(kt * 8 + c8));
        }
#pragma unroll
        for (int i = 0; i < 2 * NR; ++i) {
            const int id = tid + LW_THREADS * i, r = id >> 3, c8 = id & 7;
            ga[i] = *reinterpret_cast<const v4u_t*>(A + (size_t)r * a.lda + kt * 64 + c8 * 8);
        }
    };
    auto lstore = [&](int buf) {
        char* bp = smem + buf * BUF;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + LW_THREADS * i, r = id >> 3, c8 = id & 7;
            *reinterpret_cast<v4u_t*>(bp + lds_chunk_off(r, c8)) = drop_chunk16<T>(gx[i], keep[i], d.scale);
        }
#pragma unroll
        for (int i = 0; i < 2 * NR; ++i) {
            const int id = tid + LW_THREADS * i, r = id >> 3, c8 = id & 7;
            *reinterpret_cast<v4u_t*>(bp + lds_chunk_off(64 + r, c8)) = ga[i];
        }
    };

    f32x16 acc[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

    const int xrow = wm * 32 + l31, arow = 64 + wn * (Rp / 2) + l31;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int k = 0; k < a.nk; ++k) {
        const int buf = k & 1;
        const bool more = k + 1 < a.nk;               // uniform
        if (more) gload(k + 1);
        const char* bp = smem + buf * BUF;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int chunk = ks * 2 + hi;
            const uint4 xf = *reinterpret_cast<const uint4*>(bp + lds_chunk_off(xrow, chunk));
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const uint4 af = *reinterpret_cast<const uint4*>(bp + lds_chunk_off(arow + j * 32, chunk));
                acc[j] = Mfma32x32x16<T>::run(af, xf, acc[j]);
            }
        }
        if (more) lstore(buf ^ 1);                    // last read in K-step k - 1, which every wave left at the barrier below
        __syncthreads();
    }

    // acc[j][4 q + e] = u[m0 + wm * 32 + l31][g Rp + wn * Rp / 2 + j * 32 + 8 q + 4 hi + e]
    T* __restrict__ u = reinterpret_cast<T*>(a.u) + (size_t)(m0 + wm * 32 + l31) * a.ldu + g * Rp + wn * (Rp / 2) + 4 * hi;
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float v[4] = {acc[j][4 * q], acc[j][4 * q + 1], acc[j][4 * q + 2], acc[j][4 * q + 3]};
            store4<T>(u + j * 32 + 8 * q, v);
        }
}

// out = T(alpha * (ws[0] + ws[1] + ... + ws[S - 1]) (+ fp32(out) when accumulate)), 32 (f) x 32 (r) per workgroup; the transposed store goes through LDS so that
// both sides run along rows
template <typename T, bool TRANSPOSED>
__global__ __launch_bounds__(256) void lora_wgrad_reduce_kernel(const float* __restrict__ ws, int S, int F, int R, int R_out, float alpha, T* __restrict__ out,
                                                                int ld_out, int accumulate) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int f0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int fl = ty + 8 * p, f = f0 + fl, r = r0 + tx;
        float s = 0.f;
        if (r < R_out)
            for (int sl = 0; sl < S; ++sl) s += ws[((size_t)sl * F + f) * R + r];
        s *= alpha;
        if constexpr (TRANSPOSED) tile[fl][tx] = s;
        else if (r < R_out) {
            if (accumulate) s += to_f32(out[(size_t)f * ld_out + r]);
            out[(size_t)f * ld_out + r] = from_f32<T>(s);
        }
    }
    if constexpr (TRANSPOSED) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int rl = ty + 8 * p, r = r0 + rl;
            if (r < R_out) {
                float s = tile[tx][rl];
                if (accumulate) s += to_f32(out[(size_t)r * ld_out + f0 + tx]);
                out[(size_t)r * ld_out + f0 + tx] = from_f32<T>(s);
            }
        }
    }
}

bool lora_wgrad_ok(int dtype, int ld_big, int ld_small, int rows, int F, int R, int R_out, int transposed, int ld_out) {
    return (dtype == kBF16 || dtype == kF16) && rows > 0 && F > 0 && rows % 64 == 0 && F % 64 == 0 && (R == 64 || R == 128 || R == 192 || R == 256) && R_out >= 1 &&
           R_out <= R && ld_big >= F && ld_small >= R && ld_big % 8 == 0 && ld_small % 8 == 0 && ld_out >= (transposed ? F : R_out) &&
           (size_t)rows * ld_big * 2 < ((size_t)1 << 32) && (size_t)rows * ld_small * 2 < ((size_t)1 << 32);
}

// Row slices of a launch: as many as fill the chip about twice over with F / 64 column tiles, each slice LW_MIN_KSTEPS K-steps or more; a caller's count is
// kept, up to one K-step per slice.
int lora_wgrad_slices(int rows, int F, int n_slices) {
    const int nk = rows / 64, tiles = F / 64;
    int S = n_slices;
    if (S <= 0) {
        int dev = 0, cus = 0;                             // of the CURRENT device, asked each time (a host-side attribute read): a process may drive several
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        S = cdiv(2 * cus, tiles);
        const int most = nk / LW_MIN_KSTEPS;
        if (S > most) S = most;
    }
    if (S > nk) S = nk;
    return S < 1 ? 1 : S;
}

size_t lora_wgrad_workspace_bytes(int rows, int F, int R, int n_slices) {
    return (size_t)lora_wgrad_slices(rows, F, n_slices) * (size_t)F * (size_t)R * sizeof(float);
}

namespace {

// R >= 192 needs 64 KiB of LDS or more.  The opt-in belongs to the device that is current when it is made: once per device, not once per process.
void opt_in_large_lds() {
    int dev = 0;
    LMX_CHECK_HIP(hipGetDevice(&dev));
    static std::mutex mu;
    static uint64_t opted = 0;                            // bit d: device d has the opt-in (devices past 63 repeat it on every call)
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 0 || dev >= 64 || !(opted >> dev & 1)) {
        auto opt = [](const void* f, int bytes) { LMX_CHECK_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)); };
        opt(reinterpret_cast<const void*>(lora_wgrad_kernel<bf16_t, 3>), lw_lds_bytes(3));
        opt(reinterpret_cast<const void*>(lora_wgrad_kernel<f16_t, 3>), lw_lds_bytes(3));
        opt(reinterpret_cast<const void*>(lora_wgrad_kernel<bf16_t, 4>), lw_lds_bytes(4));
        opt(reinterpret_cast<const void*>(lora_wgrad_kernel<f16_t, 4>), lw_lds_bytes(4));
        opt(reinterpret_cast<const void*>(lora_wgrad_drop_kernel<bf16_t, 3>), lw_lds_bytes(3));
        opt(reinterpret_cast<const void*>(lora_wgrad_drop_kernel<f16_t, 3>), lw_lds_bytes(3));
        opt(reinterpret_cast<const void*>(lora_wgrad_drop_kernel<bf16_t, 4>), lw_lds_bytes(4));
        opt(reinterpret_cast<const void*>(lora_wgrad_drop_kernel<f16_t, 4>), lw_lds_bytes(4));
        opt(reinterpret_cast<const void*>(lora_down_dropout_kernel<bf16_t, 3>), ld_lds_bytes(3));
        opt(reinterpret_cast<const void*>(lora_down_dropout_kernel<f16_t, 3>), ld_lds_bytes(3));
        opt(reinterpret_cast<const void*>(lora_down_dropout_kernel<bf16_t, 4>), ld_lds_bytes(4));
        opt(reinterpret_cast<const void*>(lora_down_dropout_kernel<f16_t, 4>), ld_lds_bytes(4));
        if (dev >= 0 && dev < 64) opted |= (uint64_t)1 << dev;
    }
}

// drop = null: the plain product; else the mask of *drop on the big operand
void lora_wgrad_impl(int dtype, const void* big, int ld_big, const void* small, int ld_small, int rows, int F, int R, int R_out, float alpha, int transposed,
                     int n_slices, void* out, int ld_out, void* workspace, size_t workspace_bytes, const DropSpec* drop, bool accumulate, hipStream_t st) {
    dispatch_dtype16(dtype, "lora_wgrad", [&](auto t) {      // first: the shape rule below would report a bad dtype code as a bad shape
        using T = LMX_T(t);
        LMX_REQUIRE(lora_wgrad_ok(dtype, ld_big, ld_small, rows, F, R, R_out, transposed, ld_out),
                    "lora_wgrad: 16-bit operands, rows and F multiples of 64, R one of 64 / 128 / 192 / 256, 1 <= R_out <= R, 16-byte aligned row strides, "
                    "operands below 4 GiB");
        LMX_REQUIRE(big && small && out && workspace, "lora_wgrad: null argument");
        LMX_REQUIRE(((uintptr_t)big & 15) == 0 && ((uintptr_t)small & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out & 1) == 0,
                    "lora_wgrad: operands and workspace must be 16-byte aligned");
        LMX_REQUIRE(n_slices >= 0, "lora_wgrad: n_slices must be 0 (automatic) or positive");
        const int S = lora_wgrad_slices(rows, F, n_slices);
        LMX_REQUIRE(workspace_bytes >= (size_t)S * F * R * sizeof(float), "lora_wgrad: workspace smaller than lmx_op_lora_wgrad_workspace reports");
        LoraWgradDropArgs a{};
        a.big = big; a.small = small; a.ws = reinterpret_cast<float*>(workspace);
        a.ld_big = ld_big; a.ld_small = ld_small; a.F = F; a.nk = rows / 64; a.S = S;
        if (drop) a.d = *drop;
        const LoraWgradArgs& plain = a;
        opt_in_large_lds();
        const dim3 grid((unsigned)((F / 64) * S));
        const int NR = R / 64;
        if (drop) {
            if (NR == 1) LMX_LAUNCH((lora_wgrad_drop_kernel<T, 1>), grid, dim3(LW_THREADS), lw_lds_bytes(1), st, a);
            else if (NR == 2) LMX_LAUNCH((lora_wgrad_drop_kernel<T, 2>), grid, dim3(LW_THREADS), lw_lds_bytes(2), st, a);
            else if (NR == 3) LMX_LAUNCH((lora_wgrad_drop_kernel<T, 3>), grid, dim3(LW_THREADS), lw_lds_bytes(3), st, a);
            else LMX_LAUNCH((lora_wgrad_drop_kernel<T, 4>), grid, dim3(LW_THREADS), lw_lds_bytes(4), st, a);
        } else {
            if (NR == 1) LMX_LAUNCH((lora_wgrad_kernel<T, 1>), grid, dim3(LW_THREADS), lw_lds_bytes(1), st, plain);
            else if (NR == 2) LMX_LAUNCH((lora_wgrad_kernel<T, 2>), grid, dim3(LW_THREADS), lw_lds_bytes(2), st, plain);
            else if (NR == 3) LMX_LAUNCH((lora_wgrad_kernel<T, 3>), grid, dim3(LW_THREADS), lw_lds_bytes(3), st, plain);
            else LMX_LAUNCH((lora_wgrad_kernel<T, 4>), grid, dim3(LW_THREADS), lw_lds_bytes(4), st, plain);
        }
        LMX_CHECK_HIP(hipGetLastError());
        const dim3 rgrid((unsigned)(F / 32), (unsigned)cdiv(R_out, 32));
        T* o = reinterpret_cast<T*>(out);
        if (transposed) hipLaunchKernelGGL((lora_wgrad_reduce_kernel<T, true>), rgrid, dim3(256), 0, st, a.ws, S, F, R, R_out, alpha, o, ld_out, (int)accumulate);
        else hipLaunchKernelGGL((lora_wgrad_reduce_kernel<T, false>), rgrid, dim3(256), 0, st, a.ws, S, F, R, R_out, alpha, o, ld_out, (int)accumulate);
        LMX_CHECK_HIP(hipGetLastError());
    });
}

}  // namespace

void launch_lora_wgrad(int dtype, const void* big, int ld_big, const void* small, int ld_small, int rows, int F, int R, int R_out, float alpha, int transposed,
                       int n_slices, void* out, int ld_out, void* workspace, size_t workspace_bytes, bool accumulate, hipStream_t st) {
    lora_wgrad_impl(dtype, big, ld_big, small, ld_small, rows, F, R, R_out, alpha, transposed, n_slices, out, ld_out, workspace, workspace_bytes, nullptr, accumulate, st);
}

void launch_lora_wgrad_dropout(int dtype, const void* big, int ld_big, const void* small, int ld_small, int rows, int F, int R, int R_out, float alpha,
                               int transposed, int n_slices, void* out, int ld_out, void* workspace, size_t workspace_bytes, double p, uint64_t seed, uint32_t step,
                               uint32_t stream, bool accumulate, hipStream_t st) {
    LMX_REQUIRE(p >= 0.0 && p < 1.0, "lora_wgrad_dropout: p must be in [0, 1)");
    const DropSpec d = make_drop_spec(p, seed, step, stream);
    lora_wgrad_impl(dtype, big, ld_big, small, ld_small, rows, F, R, R_out, alpha, transposed, n_slices, out, ld_out, workspace, workspace_bytes, &d, accumulate, st);
}

bool lora_down_dropout_ok(int dtype, int ldx, int lda, int ldu, int rows, int K, int Rp, int G) {
    return (dtype == kBF16 || dtype == kF16) && rows > 0 && K > 0 && rows % 64 == 0 && K % 64 == 0 && (Rp == 64 || Rp == 128 || Rp == 192 || Rp == 256) && G >= 1 &&
           G <= 3 && ldx >= K && lda >= K && ldu >= G * Rp && ldx % 8 == 0 && lda % 8 == 0 && ldu % 8 == 0;
}

void launch_lora_down_dropout(int dtype, const void* x, int ldx, const void* A, int lda, void* u, int ldu, int rows, int K, int Rp, int G, double p, uint64_t seed,
                              uint32_t step, uint32_t stream0, hipStream_t st) {
    dispatch_dtype16(dtype, "lora_down_dropout", [&](auto t) {
        using T = LMX_T(t);
        LMX_REQUIRE(lora_down_dropout_ok(dtype, ldx, lda, ldu, rows, K, Rp, G),
                    "lora_down_dropout: 16-bit operands, rows and K multiples of 64, Rp one of 64 / 128 / 192 / 256, 1 <= G <= 3, 16-byte aligned row strides");
        LMX_REQUIRE(p >= 0.0 && p < 1.0, "lora_down_dropout: p must be in [0, 1)");
        LMX_REQUIRE(x && A && u && ((uintptr_t)x & 15) == 0 && ((uintptr_t)A & 15) == 0 && ((uintptr_t)u & 15) == 0, "lora_down_dropout: operands must be 16-byte aligned");
        LoraDownArgs a{};
        a.x = x; a.A = A; a.u = u;
        a.ldx = ldx; a.lda = lda; a.ldu = ldu; a.rtiles = rows / 64; a.nk = K / 64; a.G = G;
        a.d = make_drop_spec(p, seed, step, stream0);
        opt_in_large_lds();
        const dim3 grid((unsigned)(cdiv(a.rtiles, 8) * 8 * G));
        const int NR = Rp / 64;
        if (NR == 1) LMX_LAUNCH((lora_down_dropout_kernel<T, 1>), grid, dim3(LW_THREADS), ld_lds_bytes(1), st, a);
        else if (NR == 2) LMX_LAUNCH((lora_down_dropout_kernel<T, 2>), grid, dim3(LW_THREADS), ld_lds_bytes(2), st, a);
        else if (NR == 3) LMX_LAUNCH((lora_down_dropout_kernel<T, 3>), grid, dim3(LW_THREADS), ld_lds_bytes(3), st, a);
        else LMX_LAUNCH((lora_down_dropout_kernel<T, 4>), grid, dim3(LW_THREADS), ld_lds_bytes(4), st, a);
        LMX_CHECK_HIP(hipGetLastError());
    });
}

}  // namespace lmx
