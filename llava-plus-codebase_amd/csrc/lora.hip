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

constexpr int lw_lds_bytes(int NR) { return 2 * LW_BIG_BYTES * (1 + NR); }

// byte offset of the 16-byte chunk (row r of the K-step, columns 8 c8 .. + 7) in an image whose group of 4 rows takes rg bytes
__device__ __forceinline__ int lw_chunk_off(int r, int c8, int rg) { return (r >> 2) * rg + (c8 >> 1) * 128 + (r & 3) * 32 + (c8 & 1) * 16; }

}  // namespace

template <typename T, int NR>
__global__ __launch_bounds__(LW_THREADS) void lora_wgrad_kernel(LoraWgradArgs a) {
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
    auto gload = [&](int kt) {
        const size_t row0 = (size_t)kt * 64;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + LW_THREADS * i, r = id >> 3, c8 = id & 7;
            gb[i] = *reinterpret_cast<const v4u_t*>(big + (row0 + r) * a.ld_big + f0 + c8 * 8);
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

// out = T(alpha * (ws[0] + ws[1] + ... + ws[S - 1])), 32 (f) x 32 (r) per workgroup; the transposed store goes through LDS so that both sides run along rows
template <typename T, bool TRANSPOSED>
__global__ __launch_bounds__(256) void lora_wgrad_reduce_kernel(const float* __restrict__ ws, int S, int F, int R, int R_out, float alpha, T* __restrict__ out,
                                                                int ld_out) {
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
        else if (r < R_out) out[(size_t)f * ld_out + r] = from_f32<T>(s);
    }
    if constexpr (TRANSPOSED) {
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int rl = ty + 8 * p, r = r0 + rl;
            if (r < R_out) out[(size_t)r * ld_out + f0 + tx] = from_f32<T>(tile[tx][rl]);
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

void launch_lora_wgrad(int dtype, const void* big, int ld_big, const void* small, int ld_small, int rows, int F, int R, int R_out, float alpha, int transposed,
                       int n_slices, void* out, int ld_out, void* workspace, size_t workspace_bytes, hipStream_t st) {
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
        LoraWgradArgs a{};
        a.big = big; a.small = small; a.ws = reinterpret_cast<float*>(workspace);
        a.ld_big = ld_big; a.ld_small = ld_small; a.F = F; a.nk = rows / 64; a.S = S;
        // R >= 192 needs more than 64 KiB of LDS.  The opt-in belongs to the device that is current when it is made: once per device, not once per process.
        int dev = 0;
        LMX_CHECK_HIP(hipGetDevice(&dev));
        static std::mutex mu;
        static uint64_t opted = 0;                        // bit d: device d has the opt-in (devices past 63 repeat it on every call)
        std::lock_guard<std::mutex> lock(mu);
        if (dev < 0 || dev >= 64 || !(opted >> dev & 1)) {
            LMX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lora_wgrad_kernel<bf16_t, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, lw_lds_bytes(3)));
            LMX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lora_wgrad_kernel<f16_t, 3>), hipFuncAttributeMaxDynamicSharedMemorySize, lw_lds_bytes(3)));
            LMX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lora_wgrad_kernel<bf16_t, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, lw_lds_bytes(4)));
            LMX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lora_wgrad_kernel<f16_t, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, lw_lds_bytes(4)));
            if (dev >= 0 && dev < 64) opted |= (uint64_t)1 << dev;
        }
        const dim3 grid((unsigned)((F / 64) * S));
        const int NR = R / 64;
        if (NR == 1) LMX_LAUNCH((lora_wgrad_kernel<T, 1>), grid, dim3(LW_THREADS), lw_lds_bytes(1), st, a);
        else if (NR == 2) LMX_LAUNCH((lora_wgrad_kernel<T, 2>), grid, dim3(LW_THREADS), lw_lds_bytes(2), st, a);
        else if (NR == 3) LMX_LAUNCH((lora_wgrad_kernel<T, 3>), grid, dim3(LW_THREADS), lw_lds_bytes(3), st, a);
        else LMX_LAUNCH((lora_wgrad_kernel<T, 4>), grid, dim3(LW_THREADS), lw_lds_bytes(4), st, a);
        LMX_CHECK_HIP(hipGetLastError());
        const dim3 rgrid((unsigned)(F / 32), (unsigned)cdiv(R_out, 32));
        T* o = reinterpret_cast<T*>(out);
        if (transposed) hipLaunchKernelGGL((lora_wgrad_reduce_kernel<T, true>), rgrid, dim3(256), 0, st, a.ws, S, F, R, R_out, alpha, o, ld_out);
        else hipLaunchKernelGGL((lora_wgrad_reduce_kernel<T, false>), rgrid, dim3(256), 0, st, a.ws, S, F, R, R_out, alpha, o, ld_out);
        LMX_CHECK_HIP(hipGetLastError());
    });
}

}  // namespace lmx
