// bf16 GEMM on the gfx950 matrix cores (precision mode 2): C = epilogue(bf16(A)[M,K] * bf16(W)[N,K]^T), fp32 accumulation.
//
// One v_mfma_f32_32x32x16_bf16 per product where the f16x3 split issues three, and 2 bytes per weight element.  The operands
// are rounded to nearest-even by a plain cast (v_cvt_pk_bf16_f32 on gfx950: a NaN stays a NaN).  Activations stay fp32 in HBM:
// A is read as fp32 and rounded once while it is staged into LDS; W comes from the model's bf16 copy (launch_pack_bf16, same
// row layout as the fp32 weight, ld = K).  Bias, activation, gate, residual and the split-K reduce stay fp32 (the epilogue and the
// reduce pass are the f32 path's own).
//
// Staging per 32-deep K step: global -> registers -> LDS [rows][32 + 8] bf16 (80-byte rows: the ds_read_b128 fragment reads of 16
// consecutive rows fall on 16 distinct 4-bank groups), double-buffered, one barrier per step.  Two MFMAs per step per 32x32
// sub-tile: k-substep s of lane (r, h) holds k in [16s + 8h, 16s + 8h + 8) of row r, for both operands (cdna_hip_programming §3).
// The weight fragment is the MFMA's A operand, so the accumulator is C^T: the f32 path's epilogue_tile32 / partial_tile32 apply.
//
// It covers every GemmArgs form of the f32 path: conv-window lda, amode 1 (grouped positional conv window), grid.z batching,
// cmap / gmap row maps, gate, residual aliasing C, bias, the 4 activations and split-K partials.
#include "common.h"
#include "gemm_tile.h"

namespace artalk {

typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

// TAG only separates instantiations: launches captured into the AR/VAE hipGraph use TAG=1 (profiling: one symbol per role)
template <int BM, int BN, int WM, int WN, int AMODE, int TAG = 0>
__global__ __launch_bounds__(256, 2) void gemm_bf16_kernel(const GemmArgs g) {
    constexpr int BK = 32, LDS_LD = BK + 8;                  // bf16 elements per LDS row
    constexpr int A_TPR = BK / 4, A_RPP = 256 / A_TPR;       // A: fp32, 4 per thread (16-byte loads)
    constexpr int B_TPR = BK / 8, B_RPP = 256 / B_TPR;       // W: bf16, 8 per thread (16-byte loads)
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int A_LD = BM / A_RPP, B_LD = BN / B_RPP;
    static_assert(WM * WN == 4 && TM >= 1 && TN >= 1 && A_LD >= 1 && B_LD >= 1, "tile config");
    extern __shared__ __attribute__((aligned(16))) __bf16 smem_bf16[];
    __bf16* As = smem_bf16;                       // [2][BM][LDS_LD]
    __bf16* Bs = smem_bf16 + 2 * BM * LDS_LD;     // [2][BN][LDS_LD]

    const int tid = threadIdx.x;
    const int tiles_n = (g.N + BN - 1) / BN, tiles_m = (g.M + BM - 1) / BM;
    int tm, tn;
    tile_order(gridDim.x, blockIdx.x, tiles_m, tiles_n, (BM >= 128) ? 4 : 8, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int z = blockIdx.z;
    const float* __restrict__ A = g.A + z * g.sA;
    const __bf16* __restrict__ W = reinterpret_cast<const __bf16*>(g.Wb) + z * g.sW;

    f32x4 ra[A_LD];
    bf16x8_t rb[B_LD];
    const int arow = tid / A_TPR, ac4 = (tid % A_TPR) * 4;
    const int brow = tid / B_TPR, bc8 = (tid % B_TPR) * 8;

    auto gload = [&](int kt) {
        const int k = kt * BK + ac4;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const int gm = m0 + arow + i * A_RPP;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gm < g.M) {
                if (AMODE == 0) {
                    v = *reinterpret_cast<const f32x4*>(A + (long)gm * g.lda + k);
                } else {
                    long off;
                    if (window_src(g, gm, k, off)) v = *reinterpret_cast<const f32x4*>(A + off);
                }
            }
            ra[i] = v;
        }
        const int kb = kt * BK + bc8;
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const int gn = n0 + brow + i * B_RPP;
            bf16x8_t v = {};
            if (gn < g.N) v = *reinterpret_cast<const bf16x8_t*>(W + (long)gn * g.ldw + kb);
            rb[i] = v;
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            bf16x4_t v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (__bf16)ra[i][e];      // round to nearest even (v_cvt_pk_bf16_f32)
            *reinterpret_cast<bf16x4_t*>(As + (buf * BM + arow + i * A_RPP) * LDS_LD + ac4) = v;
        }
#pragma unroll
        for (int i = 0; i < B_LD; ++i)
            *reinterpret_cast<bf16x8_t*>(Bs + (buf * BN + brow + i * B_RPP) * LDS_LD + bc8) = rb[i];
    };

    const int wave = tid >> 6, lane = tid & 63;
    const int wm = wave / WN, wn = wave % WN;
    const int r = lane & 31, h = lane >> 5;

    f32x16 acc[TM][TN];
    zero_acc(acc);

    // K % 32 == 0 (callers); split-K: this workgroup owns K steps [kt0, nk)
    int kt0, nkt;
    k_range(g.K / BK, blockIdx.y, g.splitk, kt0, nkt);
    const int nk = kt0 + nkt;
    if (kt0 < nk) {
        gload(kt0);
        lstore(0);
    }
    __syncthreads();
    for (int kt = kt0; kt < nk; ++kt) {
        const int buf = (kt - kt0) & 1;
        if (kt + 1 < nk) gload(kt + 1);
        const __bf16* as = As + (buf * BM + wm * (BM / WM) + r) * LDS_LD + h * 8;
        const __bf16* bs = Bs + (buf * BN + wn * (BN / WN) + r) * LDS_LD + h * 8;
        bf16x8_t a[TM][2], b[TN][2];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s) a[i][s] = *reinterpret_cast<const bf16x8_t*>(as + i * 32 * LDS_LD + s * 16);
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int s = 0; s < 2; ++s) b[j][s] = *reinterpret_cast<const bf16x8_t*>(bs + j * 32 * LDS_LD + s * 16);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[j][s], a[i][s], acc[i][j], 0, 0, 0);   // C^T: epilogue_tile32
        if (kt + 1 < nk) lstore(buf ^ 1);
        __syncthreads();
    }

    if (g.splitk > 1) {   // raw partial sums; bias/act/gate/residual are applied by splitk_reduce_kernel
        float* __restrict__ P = g.partial + (long)blockIdx.y * g.M * g.N;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) partial_tile32(g, P, m0 + wm * (BM / WM) + i * 32 + r, n0 + wn * (BN / WN) + j * 32, h, acc[i][j]);
        return;
    }
    const EpiCtx epi = make_epi(g, g.bias ? g.bias + z * g.sBias : nullptr, g.C + z * g.sC, g.R ? g.R + z * g.sR : nullptr);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) epilogue_tile32<false>(g, epi, m0 + wm * (BM / WM) + i * 32 + r, n0 + wn * (BN / WN) + j * 32, h, acc[i][j]);
}

template <int BM, int BN, int WM, int WN>
static void launch_bf16_cfg(const GemmArgs& g, hipStream_t s) {
    const int tiles = ((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN);
    const size_t lds = 2 * (BM + BN) * (32 + 8) * sizeof(__bf16);
    dim3 grid(tiles, g.splitk, g.batch);
    if (g.amode == 1) ARTALK_LAUNCH((gemm_bf16_kernel<BM, BN, WM, WN, 1>), grid, dim3(256), lds, s, g);
    else if (g.graph_tag) ARTALK_LAUNCH((gemm_bf16_kernel<BM, BN, WM, WN, 0, 1>), grid, dim3(256), lds, s, g);
    else ARTALK_LAUNCH((gemm_bf16_kernel<BM, BN, WM, WN, 0>), grid, dim3(256), lds, s, g);
}

// Tile choice:
//   1: 128x128 (four 32x32 accumulators per wave)  grids of >= kBf16BigTiles 128-tiles: encoder q|k|v / out / FFN, feature projection,
//                                                  conv1-6, AdaLN table (the GEMMs gemm_p8_big_kernel takes in f16x3 mode; a persistent
//                                                  LDS-DMA form of this mode is not built)
//   0: 64x64                                       smaller grids with M > 32 (AR / VAE steps, split-K), grouped positional conv
//   2: 32x128                                      M <= 32
constexpr int kBf16BigTiles = 256;
int gemm_bf16_config(const GemmArgs& g) {
    if (g.force_cfg >= 0) return g.force_cfg;
    if (g.amode == 1) return 0;
    const long t128 = (long)((g.M + 127) / 128) * ((g.N + 127) / 128);
    if (t128 >= kBf16BigTiles) return 1;
    if (g.M > 32) return 0;
    return 2;
}
int gemm_bf16_tile_count(const GemmArgs& g) {
    int bm = 64, bn = 64;
    switch (gemm_bf16_config(g)) {
        case 1: bm = 128; bn = 128; break;
        case 2: bm = 32; bn = 128; break;
        default: break;
    }
    return ((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn);
}

void launch_gemm_bf16(const GemmArgs& g, hipStream_t s) {
    if (g.M <= 0 || g.N <= 0) return;
    switch (gemm_bf16_config(g)) {
        case 1: launch_bf16_cfg<128, 128, 2, 2>(g, s); break;
        case 2: launch_bf16_cfg<32, 128, 1, 4>(g, s); break;
        default: launch_bf16_cfg<64, 64, 2, 2>(g, s); break;
    }
}

// fp32 -> bf16 (round to nearest even; NaN stays NaN), same indexing: the bf16 copy of a weight matrix
__global__ __launch_bounds__(256) void pack_bf16_kernel(const float* __restrict__ in, __bf16* __restrict__ out, long n) {
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(in + i * 4);
        bf16x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (__bf16)v[e];
        *reinterpret_cast<bf16x4_t*>(out + i * 4) = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) out[n4 * 4 + threadIdx.x] = (__bf16)in[n4 * 4 + threadIdx.x];
}
void launch_pack_bf16(const float* in, void* out, long n, hipStream_t s) {
    if (n <= 0) return;
    const long blocks = (n / 4 + 255) / 256;
    const dim3 grid((unsigned)(blocks < 4096 ? (blocks > 0 ? blocks : 1) : 4096));
    ARTALK_LAUNCH(pack_bf16_kernel, grid, dim3(256), 0, s, in, reinterpret_cast<__bf16*>(out), n);
}

}  // namespace artalk
