// JPEG out ("JPEG out"): rgb24 frames [F][H][W][3] on the device -> baseline JPEG streams out [F][cap] and their
// lengths sizes [F], without a host wait.  Integer arithmetic throughout: the bytes are defined exactly and are the same from run to run.
//
// The restart interval is one MCU row, so every MCU row of every frame is a byte-aligned segment of its own with DC predictors 0.
// Two launches per call, whatever F:
//
//   jpeg_rows_kernel   one workgroup per (MCU row, frame).  In pieces of 252 blocks (whole MCUs for both samplings), a lane a block:
//                      colour conversion, edge padding, the 4:2:0 chroma mean, the 8 x 8 integer DCT, quantisation, zigzag into LDS;
//                      the block's bit count; a scan of the counts over the piece; the block's Huffman codes into the segment's words
//                      in scratch (big-endian bit order inside a 32-bit word).  A word that two blocks share is written with atomicOr on
//                      words the workgroup zeroed before, every other word with a plain store.  Then 1-bit padding, and the segment's
//                      bytes and its count of 0xFF bytes go to seg_bytes / seg_stuffed.
//   jpeg_pack_kernel   one workgroup per (MCU row, frame).  Sums the stuffed lengths of the frame's segments (the frame's size, and the
//                      offset of its own segment), and, when the frame fits `cap`, copies its segment behind the header with 0x00 after
//                      every 0xFF and the RSTn / EOI marker behind it.  Row 0 also copies the header and writes sizes[f]: the size, or
//                      -(the size) for a frame that does not fit, of which nothing is written.
//
// Scratch per segment is the worst case (20 bits of DC and 63 x 26 bits of AC per block): the host cannot know a smaller size without
// reading the device.  The object owns it and grows it by doubling.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "artalk_hip.h"
#include "device_mem.h"
#include "kernels.h"

namespace artalk {

namespace {

constexpr int kJpegHeader = 629;
constexpr int kPiece = 252;                 // blocks per piece: a multiple of 6 and of 3
constexpr int kBlockBits = 20 + 63 * 26;    // the longest codes: DC 9 + 11, AC 16 + 10
constexpr int kWordsPerBlock = 52;          // 52 x 32 = 1664 >= kBlockBits

// Annex K, natural order
const uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
    0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// What the kernels read besides the picture, uploaded in one block with the header it belongs to.  A code is (length << 16) | bits; length 0
// marks a symbol the tables do not have.
struct JpegTables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
    int32_t q[2][64];      // scaled tables in zigzag order
};
constexpr int kTableWords = sizeof(JpegTables) / 4;

// 8-point pass of the integer DCT: M = round(2^14 A).  Row u of M is even (u even) or odd (u odd) about its middle, so the sums run
// over x[i] +- x[7 - i]; integer sums, regrouped exactly.  out[u] = (sum + kRound) >> kShift, >> arithmetic.
template <int kRound, int kShift>
__device__ __forceinline__ void dct8(const int x[8], int out[8]) {
    const int s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
    const int d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
    out[0] = (5793 * (s0 + s1 + s2 + s3) + kRound) >> kShift;
    out[4] = (5793 * (s0 - s1 - s2 + s3) + kRound) >> kShift;
    out[2] = (7568 * (s0 - s3) + 3135 * (s1 - s2) + kRound) >> kShift;
    out[6] = (3135 * (s0 - s3) - 7568 * (s1 - s2) + kRound) >> kShift;
    out[1] = (8035 * d0 + 6811 * d1 + 4551 * d2 + 1598 * d3 + kRound) >> kShift;
    out[3] = (6811 * d0 - 1598 * d1 - 8035 * d2 - 4551 * d3 + kRound) >> kShift;
    out[5] = (4551 * d0 - 8035 * d1 + 1598 * d2 + 6811 * d3 + kRound) >> kShift;
    out[7] = (1598 * d0 - 4551 * d1 + 6811 * d2 - 8035 * d3 + kRound) >> kShift;
}

// component comp (0 Y, 1 Cb, 2 Cr) of pixel (y, x) clamped into the frame: edge padding repeats the last row and column
__device__ __forceinline__ int sample(const uint8_t* __restrict__ frame, int H, int W, int y, int x, int comp) {
    y = y < H ? y : H - 1;
    x = x < W ? x : W - 1;
    const uint8_t* p = frame + ((long)y * W + x) * 3;
    const int r = p[0], g = p[1], b = p[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__device__ __forceinline__ int bit_length(int v) { return 32 - __clz(v); }      // v >= 0; 0 -> 0

// exclusive scan of one int per lane over the 256 lanes of the workgroup; *total = the sum.  tmp: 2 x 256 ints of LDS.
__device__ __forceinline__ int block_scan(int v, int* tmp, int* total) {
    const int t = threadIdx.x;
    int* a = tmp;
    int* b = tmp + 256;
    a[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        b[t] = a[t] + (t >= o ? a[t - o] : 0);
        __syncthreads();
        int* s = a; a = b; b = s;
    }
    const int incl = a[t];
    *total = a[255];
    __syncthreads();
    return incl - v;
}

// a block's writer into the segment's words: bits go in most significant first
struct BitWriter {
    uint32_t* words;
    uint64_t acc;
    int n;           // bits in acc, counting the fill of the first word
    bool first;
    __device__ __forceinline__ void begin(uint32_t* seg, uint32_t bitpos) { words = seg + (bitpos >> 5); acc = 0; n = (int)(bitpos & 31); first = n != 0; }
    __device__ __forceinline__ void put(uint32_t bits, int len) {
        acc = (acc << len) | bits;
        n += len;
        if (n >= 32) {
            const uint32_t w = (uint32_t)(acc >> (n - 32));
            if (first) atomicOr(words, w); else *words = w;      // only the first word can hold bits of the block before
            first = false;
            ++words;
            n -= 32;
            acc &= ((uint64_t)1 << n) - 1;
        }
    }
    __device__ __forceinline__ void end() {
        if (n > 0) atomicOr(words, (uint32_t)(acc << (32 - n)));      // the block behind shares this word
    }
};

// rgb [F][H][W][3]; seg_words [F][mcuy][seg_stride] words; seg_bytes / seg_stuffed [F][mcuy]: the segment's bytes before and after stuffing
template <bool k420>
__global__ __launch_bounds__(256) void jpeg_rows_kernel(const uint8_t* __restrict__ rgb, int H, int W, int mcux, const JpegTables* __restrict__ tables,
                                                        uint32_t* __restrict__ seg_words, long seg_stride, int* __restrict__ seg_bytes,
                                                        int* __restrict__ seg_stuffed) {
    constexpr int kBpm = k420 ? 6 : 3;      // blocks per MCU
    __shared__ uint32_t s_tab[kTableWords];
    __shared__ int16_t s_coef[64 * 256];     // [k][lane]
    __shared__ int s_dc[256];
    __shared__ int s_scan[512];
    __shared__ int s_carry[3];               // the DC of the last Y, Cb, Cr block of the piece before
    const int t = threadIdx.x, row = blockIdx.x, mcuy = gridDim.x;
    const long f = blockIdx.y;
    const uint8_t* frame = rgb + f * (long)H * W * 3;
    uint32_t* seg = seg_words + (f * mcuy + row) * seg_stride;
    for (int i = t; i < kTableWords; i += 256) s_tab[i] = reinterpret_cast<const uint32_t*>(tables)[i];
    if (t < 3) s_carry[t] = 0;
    __syncthreads();
    const JpegTables& T = *reinterpret_cast<const JpegTables*>(s_tab);

    const int nb = mcux * kBpm;
    uint32_t base = 0;      // bits of the segment so far
    for (int b0 = 0; b0 < nb; b0 += kPiece) {
        const int b = b0 + t;
        const bool live = t < kPiece && b < nb;
        const int mcu = b / kBpm, j = b - mcu * kBpm;
        const int comp = k420 ? (j < 4 ? 0 : j - 3) : j;
        const int tb = comp ? 1 : 0;
        if (live) {
            int X[8][8];
            if (k420 && comp) {
                const int y0 = row * 16, x0 = mcu * 16;
#pragma unroll
                for (int y = 0; y < 8; ++y)
#pragma unroll
                    for (int x = 0; x < 8; ++x)
                        X[y][x] = ((sample(frame, H, W, y0 + 2 * y, x0 + 2 * x, comp) + sample(frame, H, W, y0 + 2 * y, x0 + 2 * x + 1, comp) +
                                    sample(frame, H, W, y0 + 2 * y + 1, x0 + 2 * x, comp) + sample(frame, H, W, y0 + 2 * y + 1, x0 + 2 * x + 1, comp) + 2) >> 2) - 128;
            } else {
                const int y0 = k420 ? row * 16 + (j >> 1) * 8 : row * 8, x0 = k420 ? mcu * 16 + (j & 1) * 8 : mcu * 8;
#pragma unroll
                for (int y = 0; y < 8; ++y)
#pragma unroll
                    for (int x = 0; x < 8; ++x) X[y][x] = sample(frame, H, W, y0 + y, x0 + x, comp) - 128;
            }
#pragma unroll
            for (int y = 0; y < 8; ++y) {      // rows: T = (X M^T + 2^10) >> 11
                int o[8];
                dct8<1 << 10, 11>(X[y], o);
#pragma unroll
                for (int u = 0; u < 8; ++u) X[y][u] = o[u];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {      // columns: U = (M T + 2^13) >> 14
                int c[8], o[8];
#pragma unroll
                for (int y = 0; y < 8; ++y) c[y] = X[y][u];
                dct8<1 << 13, 14>(c, o);
#pragma unroll
                for (int v = 0; v < 8; ++v) X[v][u] = o[v];
            }
            constexpr uint8_t zz[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                        35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
#pragma unroll
            for (int k = 0; k < 64; ++k) {
                const int U = X[zz[k] >> 3][zz[k] & 7], Q = T.q[tb][k];
                const int a = ((U < 0 ? -U : U) + 4 * Q) / (8 * Q);
                int c = U < 0 ? -a : a;
                if (k) c = c < -1023 ? -1023 : c > 1023 ? 1023 : c;      // never reached (|AC| <= 1020 before rounding): keeps the table index in range
                s_coef[k * 256 + t] = (int16_t)c;
            }
            s_dc[t] = s_coef[t];
        }
        __syncthreads();
        // the DC predictor: the block before of the same component in this segment
        int pred = 0, nbits = 0;
        if (live) {
            if (k420 && comp == 0 && j > 0) pred = s_dc[t - 1];
            else if (mcu == 0) pred = 0;
            else if (t < kBpm) pred = s_carry[comp];
            else pred = s_dc[k420 && comp == 0 ? t - 3 : t - kBpm];
            const int diff = s_coef[t] - pred;
            const int cat = bit_length(diff < 0 ? -diff : diff);
            nbits = (int)(T.dc[tb][cat] >> 16) + cat;
            int run = 0;
            for (int k = 1; k < 64; ++k) {
                const int c = s_coef[k * 256 + t];
                if (c == 0) { ++run; continue; }
                nbits += (run >> 4) * (int)(T.ac[tb][0xF0] >> 16);
                const int ac = bit_length(c < 0 ? -c : c);
                nbits += (int)(T.ac[tb][((run & 15) << 4) | ac] >> 16) + ac;
                run = 0;
            }
            if (run) nbits += (int)(T.ac[tb][0] >> 16);
        }
        int piece_bits;
        const uint32_t at = base + (uint32_t)block_scan(nbits, s_scan, &piece_bits);
        // zero the words this piece starts; the word a piece before left half full keeps its bits
        const uint32_t w0 = (base + 31) >> 5, w1 = (base + (uint32_t)piece_bits + 31) >> 5;
        for (uint32_t w = w0 + t; w < w1; w += 256) seg[w] = 0;
        __syncthreads();
        if (live) {
            BitWriter bw;
            bw.begin(seg, at);
            const int diff = s_coef[t] - pred;
            const int cat = bit_length(diff < 0 ? -diff : diff);
            const uint32_t dcode = T.dc[tb][cat];
            bw.put(((dcode & 0xffff) << cat) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1)), (int)(dcode >> 16) + cat);
            int run = 0;
            for (int k = 1; k < 64; ++k) {
                const int c = s_coef[k * 256 + t];
                if (c == 0) { ++run; continue; }
                for (; run > 15; run -= 16) bw.put(T.ac[tb][0xF0] & 0xffff, (int)(T.ac[tb][0xF0] >> 16));
                const int ac = bit_length(c < 0 ? -c : c);
                const uint32_t code = T.ac[tb][(run << 4) | ac];
                bw.put(((code & 0xffff) << ac) | ((uint32_t)(c < 0 ? c - 1 : c) & ((1u << ac) - 1)), (int)(code >> 16) + ac);
                run = 0;
            }
            if (run) bw.put(T.ac[tb][0] & 0xffff, (int)(T.ac[tb][0] >> 16));
            bw.end();
        }
        __syncthreads();
        // the last MCU of the piece carries its DCs into the next one
        if (b0 + kPiece < nb && t >= kPiece - kBpm && t < kPiece) {
            const int jj = t - (kPiece - kBpm);
            if (!k420 || jj >= 3) s_carry[k420 ? jj - 3 : jj] = s_dc[t];
        }
        base += (uint32_t)piece_bits;
        __syncthreads();
    }
    // pad with 1-bits to a whole byte
    const int nbytes = (int)((base + 7) >> 3);
    if (t == 0) {
        if (base == 0) seg[0] = 0;      // (cannot happen: every block has a DC code)
        const int pad = (int)(nbytes * 8u - base);
        if (pad) atomicOr(seg + (base >> 5), ((1u << pad) - 1) << (32 - (int)(base & 31) - pad));
    }
    __syncthreads();
    int ff = 0;
    for (int w = t; w * 4 < nbytes; w += 256) {
        const uint32_t v = seg[w];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (w * 4 + i < nbytes && ((v >> (24 - 8 * i)) & 0xff) == 0xff) ++ff;
    }
    int total;
    (void)block_scan(ff, s_scan, &total);
    if (t == 0) {
        seg_bytes[f * mcuy + row] = nbytes;
        seg_stuffed[f * mcuy + row] = nbytes + total;
    }
}

// out [F][cap]; header_dev: the kJpegHeader bytes every frame starts with
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const uint32_t* __restrict__ seg_words, long seg_stride, const int* __restrict__ seg_bytes,
                                                        const int* __restrict__ seg_stuffed, const uint8_t* __restrict__ header_dev,
                                                        uint8_t* __restrict__ out, long cap, int64_t* __restrict__ sizes) {
    __shared__ int s_scan[512];
    __shared__ long long s_sum[2][256];
    const int t = threadIdx.x, row = blockIdx.x, mcuy = gridDim.x;
    const long f = blockIdx.y;
    // the frame's size and where this segment starts: every segment is followed by two bytes, RSTn or EOI
    long long before = 0, all = 0;
    for (int r = t; r < mcuy; r += 256) {
        const long long n = seg_stuffed[f * mcuy + r] + 2;
        all += n;
        if (r < row) before += n;
    }
    s_sum[0][t] = before; s_sum[1][t] = all;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { s_sum[0][t] += s_sum[0][t + o]; s_sum[1][t] += s_sum[1][t + o]; }
        __syncthreads();
    }
    const long long total = kJpegHeader + s_sum[1][0];
    const bool fits = total <= cap;
    if (row == 0 && t == 0) sizes[f] = fits ? total : -total;
    if (!fits) return;      // (the whole workgroup: total is uniform)
    uint8_t* dst = out + f * cap;
    if (row == 0)
        for (int i = t; i < kJpegHeader; i += 256) dst[i] = header_dev[i];
    dst += kJpegHeader + s_sum[0][0];
    const uint32_t* seg = seg_words + (f * mcuy + row) * seg_stride;
    const int nbytes = seg_bytes[f * mcuy + row];
    long at = 0;      // stuffed bytes of the pieces before
    for (int p0 = 0; p0 < nbytes; p0 += 2048) {      // a lane takes 8 bytes of a piece
        const int k0 = p0 + t * 8;
        uint8_t v[8];
        int ff = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t w = k0 + 4 * h < nbytes ? seg[(k0 >> 2) + h] : 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[4 * h + i] = (uint8_t)(w >> (24 - 8 * i));
                if (k0 + 4 * h + i < nbytes && v[4 * h + i] == 0xff) ++ff;
            }
        }
        int piece_ff;
        int o = block_scan(ff, s_scan, &piece_ff);
        uint8_t* d = dst + at + (k0 - p0) + o;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (k0 + i < nbytes) {
                *d++ = v[i];
                if (v[i] == 0xff) *d++ = 0;
            }
        const int left = nbytes - p0;
        at += (left < 2048 ? left : 2048) + piece_ff;
    }
    if (t == 0) {
        dst[at] = 0xff;
        dst[at + 1] = row + 1 < mcuy ? (uint8_t)(0xd0 + (row & 7)) : (uint8_t)0xd9;
    }
}

int jpeg_mcu_side(int subsampling) { return subsampling == ARTALK_JPEG_420 ? 16 : 8; }

// {code length << 16 | code} of every symbol of an Annex K table (canonical codes, Annex C)
void fill_codes(const uint8_t bits[16], const uint8_t* vals, uint32_t* out, int n_out) {
    for (int i = 0; i < n_out; ++i) out[i] = 0;
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = (uint32_t)len << 16 | code++;
        code <<= 1;
    }
}

void scaled_table(const uint8_t base[64], int quality, uint8_t natural[64]) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int v = (base[i] * s + 50) / 100;
        natural[i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}

void put_segment(std::vector<uint8_t>& h, int marker, const std::vector<uint8_t>& payload) {
    const int len = (int)payload.size() + 2;
    h.push_back(0xff); h.push_back((uint8_t)marker); h.push_back((uint8_t)(len >> 8)); h.push_back((uint8_t)len);
    h.insert(h.end(), payload.begin(), payload.end());
}

void put_dht(std::vector<uint8_t>& h, int tc_th, const uint8_t bits[16], const uint8_t* vals, int n) {
    std::vector<uint8_t> p{(uint8_t)tc_th};
    p.insert(p.end(), bits, bits + 16);
    p.insert(p.end(), vals, vals + n);
    put_segment(h, 0xc4, p);
}

}  // namespace

int jpeg_check(int F, int H, int W, int quality, int subsampling, int64_t cap, bool have_rgb, bool have_out, bool have_sizes, std::string* err) {
    if (quality < 1 || quality > 100) { *err = "quality must be in 1..100 (got " + std::to_string(quality) + ")"; return ARTALK_EINVAL; }
    if (subsampling != ARTALK_JPEG_420 && subsampling != ARTALK_JPEG_444) {
        *err = "unknown subsampling " + std::to_string(subsampling) + " (ARTALK_JPEG_420 = 1, ARTALK_JPEG_444 = 2)";
        return ARTALK_EINVAL;
    }
    if (H < 1 || W < 1 || H > kFramesMaxSide || W > kFramesMaxSide) {
        *err = "H and W must be in 1.." + std::to_string(kFramesMaxSide) + " (got " + std::to_string(H) + " x " + std::to_string(W) + ")";
        return ARTALK_EINVAL;
    }
    if (F < 0) { *err = "F must not be negative"; return ARTALK_EINVAL; }
    if (F > 0 && (!have_rgb || !have_out || !have_sizes)) { *err = "rgb, out and sizes must not be NULL"; return ARTALK_EINVAL; }
    if (cap < kJpegHeader + 2) { *err = "cap must be at least the header and EOI, " + std::to_string(kJpegHeader + 2) + " bytes (got " + std::to_string(cap) + ")"; return ARTALK_EINVAL; }
    if (F > 65535) { *err = "at most 65535 frames a call"; return ARTALK_EINVAL; }
    return ARTALK_OK;
}

void jpeg_header(int H, int W, int quality, int subsampling, std::vector<uint8_t>* header, JpegTables* tables) {
    std::vector<uint8_t>& h = *header;
    h.clear();
    h.push_back(0xff); h.push_back(0xd8);
    put_segment(h, 0xe0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    JpegTables t;
    for (int i = 0; i < 2; ++i) {
        uint8_t natural[64];
        scaled_table(i ? kBaseChroma : kBaseLuma, quality, natural);
        std::vector<uint8_t> p{(uint8_t)i};
        for (int k = 0; k < 64; ++k) { t.q[i][k] = natural[kZigzag[k]]; p.push_back(natural[kZigzag[k]]); }
        put_segment(h, 0xdb, p);
    }
    const uint8_t hv = subsampling == ARTALK_JPEG_420 ? 0x22 : 0x11;
    put_segment(h, 0xc0, {8, (uint8_t)(H >> 8), (uint8_t)H, (uint8_t)(W >> 8), (uint8_t)W, 3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1});
    put_dht(h, 0x00, kDcLumaBits, kDcVals, 12);
    put_dht(h, 0x10, kAcLumaBits, kAcLumaVals, 162);
    put_dht(h, 0x01, kDcChromaBits, kDcVals, 12);
    put_dht(h, 0x11, kAcChromaBits, kAcChromaVals, 162);
    const int side = jpeg_mcu_side(subsampling), mcux = (W + side - 1) / side;
    put_segment(h, 0xdd, {(uint8_t)(mcux >> 8), (uint8_t)mcux});
    put_segment(h, 0xda, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    fill_codes(kDcLumaBits, kDcVals, t.dc[0], 16);
    fill_codes(kDcChromaBits, kDcVals, t.dc[1], 16);
    fill_codes(kAcLumaBits, kAcLumaVals, t.ac[0], 256);
    fill_codes(kAcChromaBits, kAcChromaVals, t.ac[1], 256);
    *tables = t;
}

int64_t jpeg_bound(int H, int W, int subsampling) {
    if (H < 1 || W < 1 || H > kFramesMaxSide || W > kFramesMaxSide || (subsampling != ARTALK_JPEG_420 && subsampling != ARTALK_JPEG_444)) return ARTALK_EINVAL;
    const int side = jpeg_mcu_side(subsampling);
    const int64_t mcux = (W + side - 1) / side, mcuy = (H + side - 1) / side;
    const int64_t seg = (mcux * (subsampling == ARTALK_JPEG_420 ? 6 : 3) * kBlockBits + 7) / 8;
    return kJpegHeader + mcuy * (2 * seg + 2);
}

}  // namespace artalk

using namespace artalk;

// One cached header: the bytes and the tables behind them in one device block
struct JpegHeaderDev {
    DevBuf<uint8_t> mem;      // [sizeof(JpegTables)] tables, then kJpegHeader bytes
};

struct artalk_jpeg {
    int device = 0;
    std::map<std::tuple<int, int, int, int>, std::unique_ptr<JpegHeaderDev>> headers;      // (H, W, quality, subsampling)
    DevBuf<uint32_t> words;      // the segments' code bits
    DevBuf<int> seg;             // [2][F mcuy]: bytes, stuffed bytes
    bool timing = false;         // time the two launches of every call: the call then waits for its last launch
    StageTimer timer;
    double launch_ms[2] = {0, 0};
    std::string err;
};

namespace {

thread_local std::string g_jpeg_error;

int jfail(artalk_jpeg* j, int rc, const std::string& msg) { (j ? j->err : g_jpeg_error) = msg; return rc; }

}  // namespace

extern "C" {

const char* artalk_jpeg_last_error(artalk_jpeg* j) { return j ? j->err.c_str() : g_jpeg_error.c_str(); }

int64_t artalk_jpeg_default_cap(int H, int W) {
    if (H < 1 || W < 1 || H > kFramesMaxSide || W > kFramesMaxSide) return ARTALK_EINVAL;
    return (int64_t)H * W * 3 + 1024;
}

int64_t artalk_jpeg_bound(int H, int W, int subsampling) { return jpeg_bound(H, W, subsampling); }

int artalk_jpeg_header(int H, int W, int quality, int subsampling, uint8_t* out_host, int out_cap) {
    std::string err;
    const int rc = jpeg_check(0, H, W, quality, subsampling, kJpegHeader + 2, false, false, false, &err);
    if (rc != ARTALK_OK || !out_host || out_cap < kJpegHeader) { g_jpeg_error = rc != ARTALK_OK ? err : "out_host must hold 629 bytes"; return ARTALK_EINVAL; }
    std::vector<uint8_t> h;
    JpegTables t;
    jpeg_header(H, W, quality, subsampling, &h, &t);
    std::memcpy(out_host, h.data(), h.size());
    return (int)h.size();
}

int artalk_op_jpeg_check(int F, int H, int W, int quality, int subsampling, int64_t cap, int have_rgb, int have_out, int have_sizes, char* msg,
                         int msg_cap) {
    std::string err;
    const int rc = jpeg_check(F, H, W, quality, subsampling, cap, have_rgb != 0, have_out != 0, have_sizes != 0, &err);
    if (msg && msg_cap > 0) { std::strncpy(msg, err.c_str(), (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; }
    return rc;
}

int artalk_jpeg_create(int device, artalk_jpeg** out) {
    if (!out) { g_jpeg_error = "out must not be NULL"; return ARTALK_EINVAL; }
    *out = nullptr;
    if (device < 0) { g_jpeg_error = "device must not be negative"; return ARTALK_EINVAL; }
    std::unique_ptr<artalk_jpeg> j(new artalk_jpeg);
    j->device = device;
    *out = j.release();
    return ARTALK_OK;
}

void artalk_jpeg_destroy(artalk_jpeg* j) {
    if (!j) return;
    DeviceGuard guard(j->device);
    delete j;
}

int artalk_jpeg_set_timing(artalk_jpeg* j, int enable) {
    if (!j) { g_jpeg_error = "the encoder must not be NULL"; return ARTALK_EINVAL; }
    j->timing = enable != 0;
    return ARTALK_OK;
}

int artalk_jpeg_get_timing(const artalk_jpeg* j, double* launch_ms, int n) {
    if (!j) { g_jpeg_error = "the encoder must not be NULL"; return ARTALK_EINVAL; }
    if (launch_ms) for (int i = 0; i < n && i < 2; ++i) launch_ms[i] = j->launch_ms[i];
    return 2;
}

int artalk_jpeg_encode(artalk_jpeg* j, const uint8_t* rgb_dev, int F, int H, int W, int quality, int subsampling, uint8_t* out_dev, int64_t cap,
                       int64_t* sizes_dev, void* stream) {
    if (!j) { g_jpeg_error = "the encoder must not be NULL"; return ARTALK_EINVAL; }
    std::string err;
    const int rc = jpeg_check(F, H, W, quality, subsampling, cap, rgb_dev != nullptr, out_dev != nullptr, sizes_dev != nullptr, &err);
    if (rc != ARTALK_OK) return jfail(j, rc, err);
    if (F == 0) return ARTALK_OK;
    DeviceGuard guard(j->device);
    hipStream_t s = (hipStream_t)stream;
    const int side = jpeg_mcu_side(subsampling), mcux = (W + side - 1) / side, mcuy = (H + side - 1) / side;
    const int64_t seg_stride = (int64_t)mcux * (subsampling == ARTALK_JPEG_420 ? 6 : 3) * kWordsPerBlock + 1;
    const size_t n_words = (size_t)F * mcuy * seg_stride, n_seg = (size_t)F * mcuy * 2;
    auto& slot = j->headers[std::make_tuple(H, W, quality, subsampling)];
    const bool waits = !slot || n_words > j->words.capacity() || n_seg > j->seg.capacity();
    if (waits) {      // an upload or a buffer that grows waits for the stream's earlier work: not inside a capture
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return jfail(j, ARTALK_EHIP, "hipStreamIsCapturing failed"); }
        if (st != hipStreamCaptureStatusNone) {
            if (!slot) j->headers.erase(std::make_tuple(H, W, quality, subsampling));
            return jfail(j, ARTALK_EINVAL, "the first artalk_jpeg_encode of a size uploads its header and grows scratch: it cannot run during stream capture");
        }
    }
    if (!slot) {
        std::vector<uint8_t> h;
        JpegTables t;
        jpeg_header(H, W, quality, subsampling, &h, &t);
        std::vector<uint8_t> both(sizeof(t) + h.size());
        std::memcpy(both.data(), &t, sizeof(t));
        std::memcpy(both.data() + sizeof(t), h.data(), h.size());
        std::unique_ptr<JpegHeaderDev> hd(new JpegHeaderDev);
        if (!hd->mem.upload(both.data(), both.size())) {
            (void)hipGetLastError();
            j->headers.erase(std::make_tuple(H, W, quality, subsampling));
            return jfail(j, ARTALK_EHIP, "the header could not be uploaded");
        }
        slot = std::move(hd);
    }
    if (!j->words.grow(n_words, 1, 1, s) || !j->seg.grow(n_seg, 1, 1, s)) return jfail(j, ARTALK_EHIP, "no device memory for the encoder's scratch");
    const JpegTables* tables = reinterpret_cast<const JpegTables*>(slot->mem.get());
    const uint8_t* header_dev = slot->mem.get() + sizeof(JpegTables);
    int* seg_bytes = j->seg.get();
    int* seg_stuffed = seg_bytes + (size_t)F * mcuy;
    const dim3 grid((unsigned)mcuy, (unsigned)F), block(256);
    j->timer.start(s, j->timing);
    j->timer.mark(-1);
    if (subsampling == ARTALK_JPEG_420)
        ARTALK_LAUNCH(jpeg_rows_kernel<true>, grid, block, 0, s, rgb_dev, H, W, mcux, tables, j->words.get(), (long)seg_stride, seg_bytes, seg_stuffed);
    else
        ARTALK_LAUNCH(jpeg_rows_kernel<false>, grid, block, 0, s, rgb_dev, H, W, mcux, tables, j->words.get(), (long)seg_stride, seg_bytes, seg_stuffed);
    j->timer.mark(0);
    ARTALK_LAUNCH(jpeg_pack_kernel, grid, block, 0, s, (const uint32_t*)j->words.get(), (long)seg_stride, (const int*)seg_bytes, (const int*)seg_stuffed,
                  header_dev, out_dev, (long)cap, sizes_dev);
    j->timer.mark(1);
    if (j->timing) { j->launch_ms[0] = j->launch_ms[1] = 0; j->timer.finish(j->launch_ms, 2); }
    if (hipGetLastError() != hipSuccess) return jfail(j, ARTALK_EHIP, "a launch failed");
    return ARTALK_OK;
}

}  // extern "C"
