// Address arithmetic shared by the GEMM kernels (gemm_f32.hip, gemm_f16s.hip, gemm_bf16.hip): tile order, split-K range, the
// positional-conv window gather, the LDS geometry and DMA piece mapping of the P8 LDS-DMA kernels, and their accumulator and
// ring-loop helpers.  Inline device functions only: no state, no kernels.  A kernel keeps its schedule (the order of reads, waits,
// barriers, MFMAs and DMA issue); what is identical by intent across kernels is stated here once.
#pragma once
#include "common.h"

namespace artalk {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---- tile order ---------------------------------------------------------------------------------------------------
// Index idx of n (a block id of a grid of n workgroups, or tile number t of n tiles in a persistent kernel) -> tile (tm, tn).
// Workgroups are dealt round-robin over the 8 XCDs (each with a private 4 MiB L2; workgroups b and b + 8 share an XCD), so first
// give each XCD a contiguous run of the tile sequence (bijective remap), then walk the sequence in groups of GM row tiles,
// column-major inside a group: the GM A-panels stay L2-resident while the W panels stream past once per group instead of once per
// row tile, and an XCD's L2 sees few distinct weight / activation rows at a time.  Placement only affects speed, never results.
// GM is the caller's constant: 8 (an XCD then works on ~8 x 4 tiles at a time), fewer for taller tiles - or ALL row tiles when
// there are few (gemm_p8_big_kernel on the AdaLN table: 23 row tiles x 222 column tiles; with groups of 8 every XCD walked all
// 222 column tiles and pulled the whole 233 MB weight matrix, 2.0 GB read per launch; column-major over all rows an XCD reads an
// eighth of it).
__device__ __forceinline__ void tile_order(int n, int idx, int tiles_m, int tiles_n, int GM, int& tm, int& tn) {
    const int xcd = idx & 7, q = n >> 3, r = n & 7;
    const int seq = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (idx >> 3);
    const int width = GM * tiles_n;
    const int group = seq / width, first_m = group * GM;
    const int gsz = min(tiles_m - first_m, GM);
    const int in_g = seq - group * width;
    tn = in_g / gsz;
    tm = first_m + (in_g - tn * gsz);
}

// split-K: workgroup y of splitk owns the nk K tiles [kt0, kt0 + nk) of nk_all (nk may be 0 when splitk > nk_all).  With splitk > 1 a kernel
// stores raw sums into slab y of g.partial; splitk_reduce[_ln768]_kernel finishes them (bias, activation, gate, residual).
__device__ __forceinline__ void k_range(int nk_all, unsigned y, int splitk, int& kt0, int& nk) {
    kt0 = (int)((long)nk_all * y / splitk);
    nk = (int)((long)nk_all * (y + 1) / splitk) - kt0;
}

// amode 1, the grouped positional-conv window (gemm_f32.hip): GEMM row gm = (chunk c, frame t), K index k = (tap, channel ci).
// Returns whether the source frame t + tap - pad lies inside the chunk (outside: the convolution's zero padding) and its element
// offset from A.
__device__ __forceinline__ bool window_src(const GemmArgs& g, int gm, int k, long& off) {
    const int c = gm / g.pc_tstride, t = gm - c * g.pc_tstride;
    const int tap = k / g.pc_cin, ci = k - tap * g.pc_cin;
    const int ts = t + tap - g.pc_pad;
    off = ((long)c * g.pc_tstride + ts) * g.lda + ci;
    return ts >= 0 && ts < g.pc_T;
}

// ---- accumulators -------------------------------------------------------------------------------------------------
template <int TM, int TN>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
}
template <int TM, int TN>
__device__ __forceinline__ void scale_acc(f32x16 (&acc)[TM][TN], float s) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] *= s;
}
// (no shared loop over partial_tile32: one more inlined level makes hipcc recompute the store address per element, +2 .. +88 instructions)
// Term t of the f16x3 product of one 16-deep k block: hi*hi, lo*hi, hi*lo (b = weight, a = activation; the order every split kernel
// accumulates in).  The weight fragment is the MFMA's A operand, so the accumulator is C^T (common.h, epilogue_tile32).
__device__ __forceinline__ void mfma3_term(int t, const f16x8& bh, const f16x8& bl, const f16x8& ah, const f16x8& al, f32x16& acc) {
    if (t == 0) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, ah, acc, 0, 0, 0);
    else if (t == 1) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl, ah, acc, 0, 0, 0);
    else acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, al, acc, 0, 0, 0);
}

// ---- P8 LDS-DMA kernels: waits and fragment reads -------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// Fragment reads and their waits are hand-placed: while an LDS-DMA is pending hipcc treats it as a FLAT access to both memories
// and turns every wait it inserts for a ds_read result into lgkmcnt(0), which drains the reads issued for the NEXT half step in
// front of MFMAs that do not need them.  The sched_barrier keeps register-only MFMAs from being hoisted above the wait.
template <int N>
__device__ __forceinline__ void wait_lgkmcnt() {
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
    __builtin_amdgcn_sched_barrier(0);
}
template <int OFF>
__device__ __forceinline__ f16x8 lds_read128(unsigned addr) {      // offset up to 65535 (the DS instructions' 16-bit immediate)
    f16x8 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
template <int UNIT>
__device__ __forceinline__ void wait_vmcnt_units(int units) {   // at most `units` groups of UNIT DMA instructions stay in flight
    static_assert(7 * UNIT <= 63, "vmcnt is a 6-bit counter");
    if (units >= 7) wait_vmcnt<7 * UNIT>();
    else if (units == 6) wait_vmcnt<6 * UNIT>();
    else if (units == 5) wait_vmcnt<5 * UNIT>();
    else if (units == 4) wait_vmcnt<4 * UNIT>();
    else if (units == 3) wait_vmcnt<3 * UNIT>();
    else if (units == 2) wait_vmcnt<2 * UNIT>();
    else if (units == 1) wait_vmcnt<UNIT>();
    else wait_vmcnt<0>();
}

// ---- P8 LDS geometry (the layout itself: file header of gemm_f16s.hip) ------------------------------------------------
// physical 16-byte chunk of logical chunk c of tile row `row`; an involution, applied to the DMA's source address and to the read
__device__ __forceinline__ int p8_phys_chunk(int row, int c) { return c ^ ((row >> 1) & 7); }
// LDS byte addresses of lane (r, h)'s fragments in stage 0, [k block][hi / lo]: A tile row arow, W tile row wrow (the W rows start
// w_base bytes into the stage).  Logical chunk of k block kb: hi = (kb * 2 + h) * 2, lo = the next one.  Further stages are
// + STAGE_BYTES, further 32-row MFMA tiles + 4096 B with the same swizzle key, which goes into the read's immediate offset.
__device__ __forceinline__ void p8_frag_offsets(unsigned lds0, int w_base, int arow, int wrow, int h, unsigned (&a_off)[2][2], unsigned (&w_off)[2][2]) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int lo = 0; lo < 2; ++lo) {
            const int c = (kb * 2 + h) * 2 + lo;
            a_off[kb][lo] = lds0 + arow * 128 + (p8_phys_chunk(arow, c) << 4);
            w_off[kb][lo] = lds0 + w_base + wrow * 128 + (p8_phys_chunk(wrow, c) << 4);
        }
}
// k block 0 only: k block 1 is the same address with bit 6 flipped (logical chunk + 4 under the XOR) - two registers per operand
__device__ __forceinline__ void p8_frag_offsets(unsigned lds0, int w_base, int arow, int wrow, int h, unsigned (&a_off)[2], unsigned (&w_off)[2]) {
#pragma unroll
    for (int lo = 0; lo < 2; ++lo) {
        const int c = h * 2 + lo;
        a_off[lo] = lds0 + arow * 128 + (p8_phys_chunk(arow, c) << 4);
        w_off[lo] = lds0 + w_base + wrow * 128 + (p8_phys_chunk(wrow, c) << 4);
    }
}
// DMA pieces: a wave-instruction copies 1 KiB = 8 tile rows x 128 B; lane = (row in piece prow = lane >> 3, physical chunk
// pchunk = lane & 7) and fetches the logical chunk that belongs there.  A wave owns `pieces` consecutive pieces of an operand's tile:
// tile row of its piece q
__device__ __forceinline__ int p8_piece_row(int wave, int pieces, int q, int prow) { return (wave * pieces + q) * 8 + prow; }
// flat source address of the lane's 16 bytes at K tile 0 (+ extra elements): operand row row0 + trow of `rows`, clamped - rows beyond the
// operand fetch the last row's bytes and are never stored
__device__ __forceinline__ const unsigned char* p8_piece_src(const void* base, int row0, int trow, int rows, int ld, int pchunk, long extra = 0) {
    const int gr = min(row0 + trow, rows - 1);
    return reinterpret_cast<const unsigned char*>(base) + ((long)gr * ld + extra) * 4 + (p8_phys_chunk(trow, pchunk) << 4);
}
// the same as a 32-bit offset into p8_rsrc's buffer, no clamp: rows beyond the operand are dropped by the hardware's range check
// and land as zeros
__device__ __forceinline__ unsigned p8_piece_off(int row0, int trow, int ld, int pchunk) {
    return (unsigned)(row0 + trow) * (unsigned)(ld * 4) + (unsigned)(p8_phys_chunk(trow, pchunk) << 4);
}
// buffer descriptor of an operand of `rows` rows: base, stride 0 (raw), bytes up to the end of the last row's K run, 32-bit data format
// (operands below 4 GiB: the launchers check)
template <class T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t p8_rsrc(const T* base, int rows, int ld, int K) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base), 0, (int)(((unsigned)(rows - 1) * (unsigned)ld + (unsigned)K) * 4u), 0x00020000);
}

// ---- the ring loop of gemm_p8_mid_kernel and gemm_p8_sm_kernel --------------------------------------------------------
// Stage 0 .. STAGES - 2 are in flight on entry (NDMA pieces per wave per stage).  Fragment registers are one half-step ahead of the
// MFMAs, so LDS-read latency and the stage hand-over (vmcnt wait + barrier) sit under matrix work instead of in front of it.
// Steady-state iteration kt (branch-free, so that hipcc counts its lgkmcnt waits exactly instead of draining at a join):
//   read kb=1 frags of stage kt | NMF MFMAs kb=0 | vmcnt: stage kt+1 landed | barrier |
//   read kb=0 frags of stage kt+1 | NMF MFMAs kb=1 with the DMA pieces of stage kt+S-1 issued one per MFMA gap
// The DMA reuses the buffer of stage kt-1, whose fragment reads were all consumed by MFMAs issued before this barrier, so no
// lgkmcnt drain is needed in front of the barrier and the kb=1 reads of stage kt stay in flight across it.
// The kernel's always-inline lambdas close over its own fragment registers: read0(buf) / read1(buf) request the k block 0 / 1
// fragments (NRD ds_read_b128 each) of ring buffer buf into register set 0 / 1, mfmas0() / mfmas1() run a set's NMF MFMAs,
// slot1(i) the i-th of set 1, issue_piece(q, kt, buf) piece q of K tile kt into buffer buf.
template <int STAGES, int NDMA, int NRD, int NMF, class R0, class R1, class M0, class M1, class S1, class IP>
__device__ __forceinline__ void p8_ring_steps(int nk, R0&& read0, R1&& read1, M0&& mfmas0, M1&& mfmas1, S1&& slot1, IP&& issue_piece) {
    wait_vmcnt_units<NDMA>(min(STAGES - 2, nk - 1));   // stage 0 landed (the prologue left up to STAGES-2 younger stages in flight)
    __builtin_amdgcn_s_barrier();
    read0(0);
    int kt = 0, buf = 0;                               // buf = kt % STAGES
    for (; kt + STAGES - 1 < nk; ++kt) {               // steady state: stage kt+S-1 still to be fetched
        const int nbuf = (buf + 1 == STAGES) ? 0 : buf + 1;
        const int fbuf = (buf == 0) ? STAGES - 1 : buf - 1;     // (kt + S - 1) % S
        read1(buf);
        wait_lgkmcnt<NRD>();                           // the kb=0 fragments (issued half a step ago) are in; the kb=1 reads fly on
        mfmas0();
        __builtin_amdgcn_sched_barrier(0);
        wait_vmcnt<(STAGES - 3) * NDMA>();             // stage kt+1 landed for this wave (stages kt+2 .. kt+S-2 may still fly)
        __builtin_amdgcn_s_barrier();                  // ... and for every wave; every wave is done with stage kt-1
        __builtin_amdgcn_sched_barrier(0);
        read0(nbuf);
        wait_lgkmcnt<NRD>();                           // kb=1 fragments of stage kt
#pragma unroll
        for (int sidx = 0; sidx < (NMF > NDMA ? NMF : NDMA); ++sidx) {
            if (sidx < NMF) slot1(sidx);
            if (sidx < NDMA) {
                __builtin_amdgcn_sched_barrier(0);
                issue_piece(sidx, kt + STAGES - 1, fbuf);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        buf = nbuf;
    }
    for (; kt < nk; ++kt) {                            // drain: the last S-1 stages are in flight or landed
        const int nbuf = (buf + 1 == STAGES) ? 0 : buf + 1;
        read1(buf);
        wait_lgkmcnt<NRD>();
        mfmas0();
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < nk) {
            wait_vmcnt_units<NDMA>(min(STAGES - 3, nk - 2 - kt));
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            read0(nbuf);
            wait_lgkmcnt<NRD>();
        } else {
            wait_lgkmcnt<0>();
        }
        mfmas1();
        __builtin_amdgcn_sched_barrier(0);
        buf = nbuf;
    }
}

}  // namespace artalk
