// Hand-written CDNA4 (gfx950) flash-attention FORWARD for MI355X.
//
// Causal, bf16, head_dim 128, arbitrary [B, H, S, D] strides (S % 64 == 0).
// One 4-wave workgroup owns one (batch, head, 64-query block); K/V tiles
// stream through LDS; Q fragments stay in registers; online softmax in
// fp32; P takes one per-wave LDS round trip to re-shape from the MFMA C
// layout to the A layout. Emits O and the logsumexp rows the aten flash
// backward consumes (torch.ops.aten._scaled_dot_product_flash_attention_
// backward), so training uses this forward + the library backward.
//
// MFMA: v_mfma_f32_16x16x32_bf16 per-wave tiles (layouts verified on
// silicon by mfma_probe in ops.hip / tests/test_ops_gpu.py):
//   A[16x32]: lane l -> A[l & 15][(l >> 4) * 8 + j]
//   B[32x16]: lane l -> B[(l >> 4) * 8 + j][l & 15]
//   C[16x16]: lane l, reg r -> C[(l >> 4) * 4 + r][l & 15]
//
// LDS layout (the v1 linear layouts measured 1113 us vs aotriton's 442 —
// every 256-B-stride row put a 16-lane read group on one bank; v2's
// transposed-V writes were 16-way write-conflicted, SQ_LDS_BANK_CONFLICT
// = 35% of wave cycles):
//   * K tile [64][128] with the guide's T2 XOR swizzle
//     (byte ^= (row & 15) << 4): contiguous uint4 staging writes and
//     conflict-free ds_read_b128 QK^T B-fragments.
//   * V transposed [d][kv] with a (d>>3)-keyed slot XOR (see vt_byte):
//     <=2-way scatter writes, single conflict-free b128 P@V B-fragment
//     reads (v4's scalar-read variant was VALU-bound on address math).
//   * P strip [16][64] with byte ^= (row & 7) << 4.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>
#include <cstdlib>
#include <cstring>

typedef unsigned short u16;
typedef unsigned int u32;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define ATTN_BM 64
#define ATTN_BN 64
#define ATTN_D 128
#define ATTN_WAVES 4
__device__ __forceinline__ u16 attn_f2bf(float f) {
  __hip_bfloat16_raw r = __float2bfloat16(f);
  return r.x;
}

__device__ __forceinline__ float bf2f_(u16 b) {
  union { u32 u; float f; } c;
  c.u = ((u32)b) << 16;
  return c.f;
}

// T2 swizzle for the K tile: 16-byte slot index XORed with row & 15.
__device__ __forceinline__ int k_byte(int row, int col_elem) {
  return (row * ATTN_D * 2 + col_elem * 2) ^ ((row & 15) << 4);
}

// Transposed V image [d][kv] with a (d>>3)-keyed slot XOR.
// Writes scatter one u16 per d (16 lanes share a kv row but have distinct
// c8 -> distinct (d>>3) -> distinct banks, <=2-way on the r halves);
// reads are one contiguous b128 of 8 kv for this lane's d (the XOR is
// constant across the 16-byte run and 36*low already spreads the lane
// group over distinct dword banks). Pitch 144 B keeps b128 16-B aligned;
// the XOR (<=240 B) may cross row ends, so the buffer carries 256 B of
// tail padding.
#define VT_PITCH_B 144
// slot-XOR key k(m), m = d>>3: (m&7) | (((m>>1)&1)<<3).
// Constraints (brute-force verified over the full image):
//  * byte-map injective: rows 8m-1/8m share a 256-B block at odd m, so
//    adjacent key pairs must flip slot-bit-3 together (the 9m key violated
//    this and corrupted the image);
//  * v6 b128 reads (32-d spans, lane groups {0-3,12-15,20-27}): <=2-way
//    (the v5 key (d>>3)&15 was 3-way there);
//  * v5 reads <=2-way, write scatter <=4-way (k mod 8 = m mod 8 spread).
__device__ __forceinline__ int vt_byte(int d, int kv) {
  const int m = d >> 3;
  return (d * VT_PITCH_B + kv * 2) ^
         ((((m & 7) | (((m >> 1) & 1) << 3))) << 4);
}

// P strip swizzle (row length 128 B = 8 slots): XOR with row & 7.
__device__ __forceinline__ int p_byte(int row, int col_elem) {
  return (row * ATTN_BN * 2 + col_elem * 2) ^ ((row & 7) << 4);
}

// ---------------------------------------------------------------------------
// Block-id decode shared by the v7 forward and the dq/dv/dk kernels, which
// launch on a 1-D grid of n_row_blocks * n_heads * batch workgroups.
//
// rank orders the row blocks by work under the causal mask, 0 = heaviest
// (fwd/dq: q block n-1-rank; dv/dk: kv block rank); one row block of rank r
// walks n_row_blocks - r units of four 64-row tile steps.
//
// LEGACY is the former 3-D grid read x-fastest: id = rank + n * (head +
// n_heads * batch). Heavy-first holds only inside each (head, batch), and
// with n % 8 == 0 a block's XCD class (id % 8: blocks dealt round-robin
// over the 8 XCDs, observed not promised) gets the same ranks for every
// (head, batch): per-class work 192 .. 80 units around a mean of 136 at
// n = 16.
//
// BALANCED is rank-major: all M = n_heads * batch pairs at rank 0, then
// all at rank 1, ... so the launch order is heavy-first globally (hence in
// every class) whoever takes the next block. When M % 8 == 0 the class is
// (id % M) % 8, and class c takes the contiguous pair range [c*M/8,
// (c+1)*M/8) of the (batch, head) order: every class holds every rank M/8
// times (equal work), and the q heads of one kv head, neighbours in that
// order, share a class - and so one L2 for that head's K/V - whenever
// n_kv_heads * batch % 8 == 0. Otherwise pairs go in plain order.
// Both are bijections of [0, n*M) for every n, n_heads, batch >= 1;
// results never depend on which is used, only speed does.
// ---------------------------------------------------------------------------

#define ATTN_SCHED_LEGACY 0
#define ATTN_SCHED_BALANCED 1

struct AttnBlock { int rank, head, batch; };

__host__ __device__ __forceinline__ AttnBlock attn_sched_block(
    unsigned id, unsigned n_row_blocks, unsigned n_heads, unsigned batch,
    int sched) {
  AttnBlock blk;
  if (sched == ATTN_SCHED_LEGACY) {
    const unsigned t = id / n_row_blocks;
    blk.rank = (int)(id - t * n_row_blocks);
    blk.batch = (int)(t / n_heads);
    blk.head = (int)(t - (unsigned)blk.batch * n_heads);
    return blk;
  }
  const unsigned M = n_heads * batch;
  const unsigned r = id / M;
  const unsigned w = id - r * M;
  const unsigned p = (M % 8 == 0) ? (w % 8) * (M / 8) + w / 8 : w;
  blk.rank = (int)r;
  blk.batch = (int)(p / n_heads);
  blk.head = (int)(p - (unsigned)blk.batch * n_heads);
  return blk;
}

// ---------------------------------------------------------------------------
// Which 32-row kv strip a wave of a dv/dk workgroup owns, and the first q
// tile the workgroup stages (used by the causal kernels only).
//
// A strip's result is one wave's chain of MFMA accumulations over (q head,
// q tile >= its rows, ascending); nothing ties the 8 waves of a workgroup
// to 8 neighbouring strips. IDENTITY is the kv block walk: workgroup rank
// owns rows [rank*256, rank*256 + 256) and walks n - rank units, 1 .. n.
// FOLD cuts the rows into 2n half-blocks of 128 and gives workgroup rank
// half-block rank (waves 0-3, heavy) and half-block 2n-1-rank (waves 4-7,
// light): a heavy and a light strip together are active in
// (4n - 2*rank) + (2*rank + 2) = 4n + 2 tile steps per q head whatever the
// rank, where two strips of the identity have 8 .. 8n. The walk starts at
// the heavy half's first tile, 2*rank; the light waves stage and reach the
// barrier but sit out the tiles before their rows. Every strip still meets
// the same tiles in the same order, so dk and dv keep their bits.
// Waves w and w+4 of a 512-thread workgroup share a SIMD (observed, not
// promised), so a SIMD runs one active wave until the walk reaches its
// light one. Pairing even with odd waves instead loses most of the gain
// (profiles/r06_dkdv_fold.md).
// ---------------------------------------------------------------------------

#define ATTN_STRIPS_IDENTITY 0
#define ATTN_STRIPS_FOLD 1

struct AttnStrips { int kv0w, qt0; };

__host__ __device__ __forceinline__ AttnStrips attn_bwd_strips(
    int fold, int rank, int wid, int n_row_blocks) {
  AttnStrips s;
  if (fold == ATTN_STRIPS_IDENTITY) {
    s.kv0w = rank * 256 + wid * 32;
    s.qt0 = rank * 4;
    return s;
  }
  const int half = wid < 4 ? rank : 2 * n_row_blocks - 1 - rank;
  s.kv0w = half * 128 + (wid & 3) * 32;
  s.qt0 = rank * 2;
  return s;
}

// ---------------------------------------------------------------------------
// PAIR: the third ownership (causal, unsplit dv/dk only; its own kernels).
//
// The fold balances the workgroups by leaving a SIMD one active wave for
// almost every tile step, and a lone wave keeps the MFMA pipe about 20 %
// busy. But a strip's chain is four chains: the accumulators of the four
// 32-column d subtiles ds are independent, each ordered only by (q head,
// q tile, q chunk c), and the S^T / dP products of a tile's two 32-row subs
// are independent too. So the two waves of a SIMD, w and w + 4, share one
// strip: wave role r = wid >> 2 computes sub r of every tile, which makes
// the packed P / dS fragments of chunks 2r and 2r + 1, the partners swap
// them through LDS, and each accumulates ds 2r and 2r + 1 over chunks
// 0 .. 3 ascending. Every accumulator meets the same fragments in the same
// order as with one owner, so dk and dv keep their bits.
//
// Workgroup rank runs two phases one after the other: half-block rank
// (heavy), then half-block 2n-1-rank (light), four strips each, walked
// from the half-block's own first tile 2*hb: (4n - 2*rank) + (2*rank + 2)
// = 4n + 2 tile steps per q head whatever the rank, both waves of every
// SIMD busy in all of them (but for the half-block's first tile, which
// strips 2 and 3 sit out).
// ---------------------------------------------------------------------------

#define ATTN_STRIPS_PAIR 2

// sub: the 32-row half of each q tile this wave computes; ds0: the first of
// the two d subtiles it accumulates; peer: the wave whose fragments it reads.
struct AttnPair { int kv0w, qt0, sub, ds0, peer; };

__host__ __device__ __forceinline__ AttnPair attn_bwd_pair(
    int rank, int phase, int wid, int n_row_blocks) {
  AttnPair p;
  const int hb = phase == 0 ? rank : 2 * n_row_blocks - 1 - rank;
  p.kv0w = hb * 128 + (wid & 3) * 32;
  p.qt0 = hb * 2;
  p.sub = wid >> 2;
  p.ds0 = (wid >> 2) * 2;
  p.peer = wid ^ 4;
  return p;
}

// Exchange area of the pair kernels: one 16-byte fragment per lane, chunk c
// of the strip that waves w and w + 4 share. Wave wid writes chunks
// 2*sub and 2*sub + 1 and reads all four back, its partner's among them.
#define ATTN_PAIR_XCH_U4 (4 * 4 * 64)        // 16 KB
__host__ __device__ __forceinline__ int attn_pair_xch(int wid, int c) {
  return ((wid & 3) * 4 + c) * 64;
}

typedef __attribute__((ext_vector_type(16))) float f32x16;

#define V6_BM 256
#define V6_QBLK 32
#define V6_BN 64
// per-buffer LDS halves (u16 counts): K [64][128] swizzled rows, then the
// transposed V image (pitch 144 B + 256 B XOR tail)
#define V6_K_U16 (V6_BN * ATTN_D)                        // 8192
#define V6_V_U16 (ATTN_D * (VT_PITCH_B / 2) + 128)       // 9344
#define V6_BUF_U16 (V6_K_U16 + V6_V_U16)

__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// raw v_exp_f32 (2^x): libm exp2f lowers to a ~5-instruction guarded
// sequence (ldexp + cndmask pairs); softmax arguments are <= 0 and
// underflow-to-0 is exactly what we want.
__device__ __forceinline__ float exp2_raw(float x) {
  float r;
  asm("v_exp_f32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

// 3-deep glds pipeline helpers (fwd v7 + the v7-style backward kernels):
// counted vmcnt only, raw barriers (no vmcnt(0) drain in any main loop)
__device__ __forceinline__ void v7_wait_vmcnt4() {
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
}
__device__ __forceinline__ void v7_wait_vmcnt0() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ void v7_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

#define V7_RING 3

// ---------------------------------------------------------------------------
// Device pieces shared by the 32x32x16 kernels (v6/v7 forward, dq, dv, dk and
// the pair kernels). All of them are lane-local in the owned row: lane
// (low = lane & 31, hi = lane >> 5) holds C[(r & 3) + 8 * (r >> 2) + 4 * hi]
// [low] in register r of an f32x16 accumulator.
// ---------------------------------------------------------------------------

#define ATTN_LOG2E 1.4426950408889634f

// one 16-byte fragment: MFMA operand, global/LDS vector, packed bf16 pairs
union AttnFrag { bf16x8 v; uint4 u; unsigned w[4]; u16 h[8]; };

// T12 repack of the 8 values s[pb .. pb+7] (pb = 0 or 8) of a C tile into
// the B fragment of its 16-row chunk: lane holds B[k = hi*8 + j][n = low]
__device__ __forceinline__ bf16x8 attn_repack(f32x16 s, int pb) {
  const unsigned a0 = cvt_pk_bf16(s[pb + 0], s[pb + 1]);
  const unsigned b0 = cvt_pk_bf16(s[pb + 4], s[pb + 5]);
  const unsigned a1 = cvt_pk_bf16(s[pb + 2], s[pb + 3]);
  const unsigned b1 = cvt_pk_bf16(s[pb + 6], s[pb + 7]);
  auto r02 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
  auto r13 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
  AttnFrag f;
  f.w[0] = r02[0];
  f.w[1] = r13[0];
  f.w[2] = r02[1];
  f.w[3] = r13[1];
  return f.v;
}

// a lane's persistent row (Q, K, V or dO) as 8 k-chunk fragments: lane
// holds row[kc*16 + hi*8 + j]
__device__ __forceinline__ void attn_load_row(AttnFrag (&f)[8],
                                              const u16* row, int hi) {
#pragma unroll
  for (int kc = 0; kc < 8; ++kc)
    f[kc].u = *reinterpret_cast<const uint4*>(row + kc * 16 + hi * 8);
}

template <int N>
__device__ __forceinline__ void attn_zero(f32x16 (&acc)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
}

// d subtile ds of a lane's row: bf16 to an output row, fp32 to a partial row
__device__ __forceinline__ void attn_store_bf16(u16* row, const f32x16& acc,
                                                int ds, int hi) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int d0 = 8 * g + 4 * hi + 32 * ds;
    uint2 wv;
    wv.x = cvt_pk_bf16(acc[4 * g + 0], acc[4 * g + 1]);
    wv.y = cvt_pk_bf16(acc[4 * g + 2], acc[4 * g + 3]);
    *reinterpret_cast<uint2*>(row + d0) = wv;
  }
}
__device__ __forceinline__ void attn_store_f32(float* row, const f32x16& acc,
                                               int ds, int hi) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int d0 = 8 * g + 4 * hi + 32 * ds;
    float4 wv;
    wv.x = acc[4 * g + 0];
    wv.y = acc[4 * g + 1];
    wv.z = acc[4 * g + 2];
    wv.w = acc[4 * g + 3];
    *reinterpret_cast<float4*>(row + d0) = wv;
  }
}

// Staging by global->LDS DMA (glds) writes lane-linear (rule 21), so the T2
// swizzle of a row image is inverted onto the SOURCE address: the 16 bytes
// that land at lane-linear byte L of a k_byte image of rows row0 .. row0+63
// come from here. The image stays byte-identical to a ds_write one and the
// XOR only permutes 16-B slots inside one 256-B row (same coalescing).
__device__ __forceinline__ const u16* attn_glds_src(const u16* base, int row0,
                                                    int L, long ss) {
  const int r = L >> 8;
  const int in = (((L & 255) ^ ((r & 15) << 4)) >> 1);
  return base + (long)(row0 + r) * ss + in;
}
// the same as an element offset into a contiguous [64, D] slab (one kv head
// of one cache page): constant per lane, whatever page a tile comes from
__device__ __forceinline__ int attn_glds_page_off(int L) {
  const int r = L >> 8;
  const int in = (((L & 255) ^ ((r & 15) << 4)) >> 1);
  return r * ATTN_D + in;
}

// Issue a thread's two 16-byte glds for each of two 64-row images,
// interleaved, and advance the sources one tile. A wave's 64 lanes land
// contiguously at img + i * HALF + woff (u16, woff wave-uniform).
template <int HALF>
__device__ __forceinline__ void attn_glds_rows2(
    u16* img_a, const u16* (&gp_a)[2], long step_a,
    u16* img_b, const u16* (&gp_b)[2], long step_b, int woff) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    __builtin_amdgcn_global_load_lds((const u32*)gp_a[i],
                                     (u32*)&img_a[i * HALF + woff], 16, 0, 0);
    gp_a[i] += step_a;
    __builtin_amdgcn_global_load_lds((const u32*)gp_b[i],
                                     (u32*)&img_b[i * HALF + woff], 16, 0, 0);
    gp_b[i] += step_b;
  }
}

// Thread tid's share of a 64-row transposed (vt_byte) image: rows rp2 and
// rp2 + 1, 8 columns from c8, written as 8 kv-pair words.
__device__ __forceinline__ void attn_write_t(char* img, const uint4& row_a,
                                             const uint4& row_b, int tid) {
  const int rp2 = (tid >> 4) * 2;
  const int c8 = (tid & 15) * 8;
  union { uint4 u; u16 h[8]; } va, vb;
  va.u = row_a;
  vb.u = row_b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const u32 pair = (u32)va.h[j] | ((u32)vb.h[j] << 16);
    *reinterpret_cast<u32*>(&img[vt_byte(c8 + j, rp2)]) = pair;
  }
}
// the same share, read back from a landed k_byte row image (LDS -> LDS)
__device__ __forceinline__ void attn_transpose(const u16* rows, char* img,
                                               int tid) {
  const char* src = reinterpret_cast<const char*>(rows);
  const int rp2 = (tid >> 4) * 2;
  const int c8 = (tid & 15) * 8;
  attn_write_t(img,
               *reinterpret_cast<const uint4*>(&src[k_byte(rp2, c8)]),
               *reinterpret_cast<const uint4*>(&src[k_byte(rp2 + 1, c8)]),
               tid);
}

// LDS of the v7 forward and of dq: a 3-slot ring of K row images, a 3-slot
// ring of V row images (both glds), then 2 transposed images built locally.
// Slot addressing by arithmetic (pointer arrays spill under pressure).
#define ATTN_RING_U16 (V7_RING * 2 * V6_K_U16 + 2 * V6_V_U16)
__device__ __forceinline__ u16* attn_ring_k(u16* lds, int slot) {
  return &lds[slot * V6_K_U16];
}
__device__ __forceinline__ u16* attn_ring_v(u16* lds, int slot) {
  return &lds[(V7_RING + slot) * V6_K_U16];
}
__device__ __forceinline__ char* attn_ring_t(u16* lds, int p) {
  return reinterpret_cast<char*>(&lds[2 * V7_RING * V6_K_U16]) +
         p * (V6_V_U16 * 2);
}

// Ring sources of thread tid: wave w stages rows 8w..8w+7 - exactly the
// rows its own lanes transpose, so the wave's own counted vmcnt covers them
// (rows staged by another wave are only guaranteed landed after a barrier).
struct AttnRingSrc {
  const u16* kgp[2];
  const u16* vgp[2];
  long kstep, vstep;
  int lslot;                                  // wave-uniform u16 base
};
__device__ __forceinline__ AttnRingSrc attn_ring_src(
    const u16* kbase, long k_ss, const u16* vbase, long v_ss, int tid) {
  AttnRingSrc s;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int L = (tid & ~63) * 32 + i * 1024 + (tid & 63) * 16;
    s.kgp[i] = attn_glds_src(kbase, 0, L, k_ss);
    s.vgp[i] = attn_glds_src(vbase, 0, L, v_ss);
  }
  s.kstep = (long)V6_BN * k_ss;
  s.vstep = (long)V6_BN * v_ss;
  s.lslot = (tid & ~63) * 16;
  return s;
}
// issue the next K and V tiles into ring slot `slot`
__device__ __forceinline__ void attn_ring_issue(u16* lds, int slot,
                                                AttnRingSrc& s) {
  attn_glds_rows2<512>(attn_ring_k(lds, slot), s.kgp, s.kstep,
                       attn_ring_v(lds, slot), s.vgp, s.vstep, s.lslot);
}


__global__ __launch_bounds__(256) void attn_fwd_kernel(
    const u16* __restrict__ q, const u16* __restrict__ k,
    const u16* __restrict__ v, u16* __restrict__ out,
    float* __restrict__ lse,
    long q_sb, long q_sh, long q_ss,
    long k_sb, long k_sh, long k_ss,
    long v_sb, long v_sh, long v_ss,
    int n_heads, int S, float scale) {
  const int qb = blockIdx.x;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int low = lane & 15;   // A/C row | B/C col within a 16-tile
  const int kg = lane >> 4;    // lane group (k chunk | C row group)

  __shared__ u16 ldsK[ATTN_BN * ATTN_D];              // swizzled rows
  __shared__ u16 ldsV[ATTN_D * (VT_PITCH_B / 2) + 128];  // transposed image
  __shared__ u16 ldsP[ATTN_WAVES][16 * ATTN_BN];      // swizzled rows

  // ---- load this wave's Q fragments (rows wid*16 .. +15) ----
  const u16* qbase = q + (long)b * q_sb + (long)h * q_sh
                     + (long)(qb * ATTN_BM) * q_ss;
  union { bf16x8 v; uint4 u; } qfrag[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    qfrag[ks].u = *reinterpret_cast<const uint4*>(
        qbase + (long)(wid * 16 + low) * q_ss + ks * 32 + kg * 8);
  }

  float m_run[4], l_run[4];
  float oacc[8][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = -INFINITY; l_run[r] = 0.f; }
#pragma unroll
  for (int ct = 0; ct < 8; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) oacc[ct][r] = 0.f;

  const u16* kbase = k + (long)b * k_sb + (long)h * k_sh;
  const u16* vbase = v + (long)b * v_sb + (long)h * v_sh;
  const int kv_end = (qb + 1) * ATTN_BM;  // causal upper bound (<= S)
  char* ldsKb = reinterpret_cast<char*>(ldsK);
  char* ldsVb = reinterpret_cast<char*>(ldsV);
  char* ldsPb = reinterpret_cast<char*>(ldsP[wid]);

  for (int kv0 = 0; kv0 < kv_end; kv0 += ATTN_BN) {
    // ---- stage K and V tiles (swizzled rows, contiguous uint4) ----
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int idx = t * 256 + threadIdx.x;
      const int r = idx >> 4;            // kv row within tile
      const int c8 = (idx & 15) * 8;     // 8-elem column chunk
      *reinterpret_cast<uint4*>(&ldsKb[k_byte(r, c8)]) =
          *reinterpret_cast<const uint4*>(
              kbase + (long)(kv0 + r) * k_ss + c8);
      union { uint4 u; u16 h[8]; } vv;
      vv.u = *reinterpret_cast<const uint4*>(
          vbase + (long)(kv0 + r) * v_ss + c8);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        *reinterpret_cast<u16*>(&ldsVb[vt_byte(c8 + j, r)]) = vv.h[j];
    }
    __syncthreads();

    // ---- S = scale * (Q @ K^T), 16x64 strip per wave ----
    f32x4 sacc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
            &ldsKb[k_byte(ct * 16 + low, ks * 32 + kg * 8)]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qfrag[ks].v, bfrag,
                                                      acc, 0, 0, 0);
      }
      sacc[ct] = acc;
    }

    // ---- causal mask + online softmax (state per reg = per C row) ----
    const int qrow0 = qb * ATTN_BM + wid * 16 + kg * 4;  // + r
    float mx[4], alpha[4], psum[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mx[r] = -INFINITY;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int col = kv0 + ct * 16 + low;
        float s = sacc[ct][r] * scale;
        if (col > qrow0 + r) s = -INFINITY;
        sacc[ct][r] = s;
        mx[r] = fmaxf(mx[r], s);
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
        mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], off, 64));
      const float mnew = fmaxf(m_run[r], mx[r]);
      alpha[r] = (m_run[r] == -INFINITY) ? 0.f : __expf(m_run[r] - mnew);
      m_run[r] = mnew;
      psum[r] = 0.f;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const float p = (sacc[ct][r] == -INFINITY)
                            ? 0.f : __expf(sacc[ct][r] - mnew);
        sacc[ct][r] = p;
        psum[r] += p;
        *reinterpret_cast<u16*>(
            &ldsPb[p_byte(kg * 4 + r, ct * 16 + low)]) = attn_f2bf(p);
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
        psum[r] += __shfl_xor(psum[r], off, 64);
      l_run[r] = l_run[r] * alpha[r] + psum[r];
#pragma unroll
      for (int ct2 = 0; ct2 < 8; ++ct2) oacc[ct2][r] *= alpha[r];
    }
    __syncthreads();  // P strips visible; K/V reads done before restage

    // ---- O += P @ V ----
    // B-fragment: ONE contiguous b128 read of 8 kv for this lane's column
    // from the transposed V image. v4's 8 scalar reads per fragment cost
    // ~14 VALU per MFMA in address math (SQ_INSTS_VALU 118.8M) — the wide
    // read removes that. (ds_read_b64_tr_b16 was probed on silicon —
    // tests/test_ops_gpu.py tr_probe — and delivers only 16 distinct
    // values per 16-lane group, so it cannot feed this fragment shape.)
#pragma unroll
    for (int ct2 = 0; ct2 < 8; ++ct2) {
      f32x4 acc = {oacc[ct2][0], oacc[ct2][1], oacc[ct2][2], oacc[ct2][3]};
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        bf16x8 afrag = *reinterpret_cast<const bf16x8*>(
            &ldsPb[p_byte(low, ks2 * 32 + kg * 8)]);
        bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
            &ldsVb[vt_byte(ct2 * 16 + low, ks2 * 32 + kg * 8)]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag, bfrag, acc,
                                                      0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) oacc[ct2][r] = acc[r];
    }
    __syncthreads();
  }

  // ---- epilogue: normalize, write O [B,H,S,D] contiguous + LSE ----
  u16* obase = out + (((long)b * n_heads + h) * S + qb * ATTN_BM
                      + wid * 16) * ATTN_D;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float inv_l = 1.0f / l_run[r];
#pragma unroll
    for (int ct2 = 0; ct2 < 8; ++ct2) {
      obase[(long)(kg * 4 + r) * ATTN_D + ct2 * 16 + low] =
          attn_f2bf(oacc[ct2][r] * inv_l);
    }
  }
  if (low == 0) {
    float* lbase = lse + ((long)b * n_heads + h) * S + qb * ATTN_BM
                   + wid * 16 + kg * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) lbase[r] = m_run[r] + __logf(l_run[r]);
  }
}

// ===========================================================================
// v6: 8-wave swapped-operand forward (guide §B "8-warp 32×32 ladder").
//
// Structure: one 512-thread workgroup owns 256 q rows (32 per wave); K/V
// tiles of 64 keys double-buffered in LDS; Q rows live in registers.
// BOTH MFMA products are operand-swapped so the q index stays lane-local
// end to end:
//   S^T = K @ Q^T   via mfma_32x32x16(A=K-frag, B=Q-frag)  -> C[kv][q=lane&31]
//   O^T = V^T @ P   via mfma_32x32x16(A=Vt-frag, B=P-frag) -> C[d][q=lane&31]
// so the online-softmax state (m, l) is one scalar pair per lane (its q row,
// 16 kv per half-wave), the row reduce is an in-register tree plus ONE
// __shfl_xor(32) half-merge, and P never round-trips through LDS
// (v5 paid a pack + ds_write + barrier + ds_read per tile for that).
// Softmax runs in exp2 space (scale2 = scale*log2e folded into the S scale).
// Techniques: T12 (cvt_pk_bf16_f32 + permlane32_swap P repack), T13
// (defer-rescale THR=8), T14 (issue next tile's global loads before QK^T,
// LDS write before PV), causal tile skip + diagonal-only masking, reversed
// qb launch order (longest blocks first), native GQA (kv head = h / group).
// ===========================================================================

template <int NW>   // waves per workgroup: 4 (BM=128, 2 WGs/CU) or 8 (BM=256)
__global__ __launch_bounds__(NW * 64) void attn_fwd_v6_kernel(
    const u16* __restrict__ q, const u16* __restrict__ k,
    const u16* __restrict__ v, u16* __restrict__ out,
    float* __restrict__ lse,
    long q_sb, long q_sh, long q_ss,
    long k_sb, long k_sh, long k_ss,
    long v_sb, long v_sh, long v_ss,
    int n_heads, int gqa_group, int S, float scale2) {
  constexpr int NT = NW * 64;          // threads
  constexpr int BM = NW * 32;          // q rows per workgroup
  constexpr int KP = 1024 / NT;        // K glds pieces per thread (16 B each)
  constexpr int VU = 512 / NT;         // V kv-pair units per thread
  const int qb = gridDim.x - 1 - blockIdx.x;   // longest-running blocks first
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int hkv = h / gqa_group;
  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int low = lane & 31;
  const int hi = lane >> 5;

  __shared__ __attribute__((aligned(16))) u16 lds[2][V6_BUF_U16];

  const int q0w = qb * BM + wid * V6_QBLK;
  const int qrow = q0w + low;                  // this lane's q row

  // Q row in registers: 8 k-chunks, lane holds Q[qrow][kc*16 + hi*8 + j]
  union F8 { bf16x8 v; uint4 u; u16 h[8]; };
  const u16* qptr = q + (long)b * q_sb + (long)h * q_sh + (long)qrow * q_ss;
  F8 qf[8];
#pragma unroll
  for (int kc = 0; kc < 8; ++kc)
    qf[kc].u = *reinterpret_cast<const uint4*>(qptr + kc * 16 + hi * 8);

  // O^T accumulators: 4 d-subtiles; lane holds O[d=crow(r,hi)+32*ds][qrow]
  f32x16 oacc[4];
#pragma unroll
  for (int ds = 0; ds < 4; ++ds)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[ds][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  const u16* kbase = k + (long)b * k_sb + (long)hkv * k_sh;
  const u16* vbase = v + (long)b * v_sb + (long)hkv * v_sh;
  const int n_tiles = (qb * BM + BM) / V6_BN;   // causal upper bound

  char* lds0 = reinterpret_cast<char*>(&lds[0][0]);
  char* lds1 = reinterpret_cast<char*>(&lds[1][0]);
  const int VOFF = V6_K_U16 * 2;               // V image byte offset in a buf

  // K staging goes by global->LDS DMA (glds): zero in-flight registers and
  // zero ds_write instructions; the T2 swizzle is inverted onto the SOURCE
  // address (rule 21: glds writes lane-linear), which keeps the LDS image
  // byte-identical to the ds_write version and costs nothing in coalescing
  // (the XOR permutes 16-B slots within one 256-B row = the same two 128-B
  // requests per 16 lanes). V cannot go by glds (transposed image) and
  // keeps register staging: kv-row pairs written as u32 after QK^T.
  const u16* kgp[KP];
  const u16* vgp[2 * VU];
#pragma unroll
  for (int i = 0; i < KP; ++i) {
    const int idx = i * NT + tid;
    const int L = idx * 16;                       // lane-linear LDS byte
    const int kr = L >> 8;
    const int kin = (((L & 255) ^ ((kr & 15) << 4)) >> 1);
    kgp[i] = kbase + (long)kr * k_ss + kin;
  }
#pragma unroll
  for (int u = 0; u < VU; ++u) {
    const int unit = u * NT + tid;                // (rp, c8) unit
    const int rp2 = (unit >> 4) * 2;
    const int c8 = (unit & 15) * 8;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      vgp[u * 2 + i] = vbase + (long)(rp2 + i) * v_ss + c8;
  }
  const long kstep = (long)V6_BN * k_ss;
  const long vstep = (long)V6_BN * v_ss;
  const int wu64 = __builtin_amdgcn_readfirstlane(tid >> 6);

  uint4 vst[2 * VU];
#define V6_GLDS_K(BUFI)                                                     \
  _Pragma("unroll")                                                         \
  for (int i = 0; i < KP; ++i) {                                            \
    __builtin_amdgcn_global_load_lds(                                       \
        (const u32*)kgp[i], (u32*)&lds[BUFI][(i * NT + wu64 * 64) * 8],     \
        16, 0, 0);                                                          \
    kgp[i] += kstep;                                                        \
  }
#define V6_LOAD_V()                                                         \
  _Pragma("unroll")                                                         \
  for (int i = 0; i < 2 * VU; ++i) {                                        \
    vst[i] = *reinterpret_cast<const uint4*>(vgp[i]);                       \
    vgp[i] += vstep;                                                        \
  }
#define V6_WRITE_V(BUF)                                                     \
  _Pragma("unroll")                                                         \
  for (int u = 0; u < VU; ++u) {                                            \
    const int unit_ = u * NT + tid;                                         \
    const int rp2_ = (unit_ >> 4) * 2;                                      \
    const int c8_ = (unit_ & 15) * 8;                                       \
    union { uint4 u4; u16 h[8]; } va_, vb_;                                 \
    va_.u4 = vst[u * 2];                                                    \
    vb_.u4 = vst[u * 2 + 1];                                                \
    _Pragma("unroll")                                                       \
    for (int j = 0; j < 8; ++j) {                                           \
      const u32 pair_ = (u32)va_.h[j] | ((u32)vb_.h[j] << 16);              \
      *reinterpret_cast<u32*>(&(BUF)[VOFF + vt_byte(c8_ + j, rp2_)]) = pair_; \
    }                                                                       \
  }

  V6_GLDS_K(0)
  V6_LOAD_V()
  V6_WRITE_V(lds0)
  __syncthreads();

  // T5 static form: the second-dispatched half of the workgroup loses
  // VALU arbitration to the older half on every segment; one setprio(1)
  // for it (wave-uniform via readfirstlane) removes its start-of-segment
  // penalty (guide: -0.8..1.5% cycles, never negative)
  if (NW == 8 && __builtin_amdgcn_readfirstlane(threadIdx.x) >= NT / 2)
    __builtin_amdgcn_s_setprio(1);

  int cur = 0;
  for (int t = 0; t < n_tiles; ++t) {
    const int kv0 = t * V6_BN;
    const bool have_next = (t + 1) < n_tiles;
    if (have_next) { V6_GLDS_K(cur ^ 1) V6_LOAD_V() }   // issue early (T14)

    char* kb = cur ? lds1 : lds0;
    char* vbuf = kb + VOFF;
    const bool active = kv0 <= q0w + V6_QBLK - 1;
    const bool need_mask = kv0 + V6_BN > q0w;

    f32x16 s0, s1;
    AttnFrag pa[4];
    float pm = -INFINITY;
    if (active) {
      // ---- S^T = K @ Q^T over 2 kv-subtiles of 32 ----
#pragma unroll
      for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
      for (int kc = 0; kc < 8; ++kc) {
        bf16x8 a0 = *reinterpret_cast<const bf16x8*>(
            &kb[k_byte(low, kc * 16 + hi * 8)]);
        s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, qf[kc].v, s0, 0, 0, 0);
        bf16x8 a1 = *reinterpret_cast<const bf16x8*>(
            &kb[k_byte(32 + low, kc * 16 + hi * 8)]);
        s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, qf[kc].v, s1, 0, 0, 0);
      }
      // ---- scale into exp2 space + causal mask + tile max ----
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kvr = kv0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          float x0 = s0[r] * scale2;
          if (kvr > qrow) x0 = -1e30f;
          s0[r] = x0;
          float x1 = s1[r] * scale2;
          if (kvr + 32 > qrow) x1 = -1e30f;
          s1[r] = x1;
          pm = fmaxf(pm, fmaxf(x0, x1));
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s0[r] *= scale2;
          s1[r] *= scale2;
          pm = fmaxf(pm, fmaxf(s0[r], s1[r]));
        }
      }
      pm = fmaxf(pm, __shfl_xor(pm, 32, 64));   // merge q-row halves
    }
    // stage tile t+1 now: QK^T covered the load latency, and writing here
    // (instead of after the P repack) ends vst's live range before the
    // softmax (the 252-VGPR scratch parking came from carrying it there)
    if (have_next) {
      char* nb = cur ? lds0 : lds1;
      V6_WRITE_V(nb)
    }
    if (active) {
      // ---- defer-rescale (T13, THR=8 in exp2 space) ----
      if (!__all(pm - m_run <= 8.0f)) {
        const float mn = fmaxf(m_run, pm);
        const float alpha = (m_run == -INFINITY) ? 0.f : exp2_raw(m_run - mn);
        m_run = mn;
        l_run *= alpha;
#pragma unroll
        for (int ds = 0; ds < 4; ++ds)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[ds][r] *= alpha;
      }
      // ---- P = exp2(s - m), row sum ----
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p0 = exp2_raw(s0[r] - m_run);
        const float p1 = exp2_raw(s1[r] - m_run);
        s0[r] = p0;
        s1[r] = p1;
        psum += p0 + p1;
      }
      psum += __shfl_xor(psum, 32, 64);
      l_run += psum;

      // ---- T12 repack: P f32 regs -> bf16 MFMA fragments, in-register ----
      // chunk c of 16 kv: lane holds P[kv = c*16 + hi*8 + j][qrow]
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
          // kept inline here: through attn_repack this kernel's <4>
          // instantiation measured 1.3 % slower
          // (profiles/r09_attention_refactor.md)
          const int pb = cc * 8;
          unsigned a0, b0, a1, b1;
          if (sub == 0) {
            a0 = cvt_pk_bf16(s0[pb + 0], s0[pb + 1]);
            b0 = cvt_pk_bf16(s0[pb + 4], s0[pb + 5]);
            a1 = cvt_pk_bf16(s0[pb + 2], s0[pb + 3]);
            b1 = cvt_pk_bf16(s0[pb + 6], s0[pb + 7]);
          } else {
            a0 = cvt_pk_bf16(s1[pb + 0], s1[pb + 1]);
            b0 = cvt_pk_bf16(s1[pb + 4], s1[pb + 5]);
            a1 = cvt_pk_bf16(s1[pb + 2], s1[pb + 3]);
            b1 = cvt_pk_bf16(s1[pb + 6], s1[pb + 7]);
          }
          auto r02 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
          auto r13 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
          AttnFrag f;
          f.w[0] = r02[0];
          f.w[1] = r13[0];
          f.w[2] = r02[1];
          f.w[3] = r13[1];
          pa[sub * 2 + cc] = f;
        }
      }

      // ---- O^T += V^T @ P over 4 kv-chunks x 4 d-subtiles ----
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) {
          bf16x8 vf = *reinterpret_cast<const bf16x8*>(
              &vbuf[vt_byte(ds * 32 + low, c * 16 + hi * 8)]);
          oacc[ds] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              vf, pa[c].v, oacc[ds], 0, 0, 0);
        }
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue: O /= l, store bf16; LSE in natural-log space ----
  const float inv_l = 1.0f / l_run;
  u16* orow = out + (((long)b * n_heads + h) * S + qrow) * ATTN_D;
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d0 = 8 * g + 4 * hi + 32 * ds;
      const unsigned w0 = cvt_pk_bf16(oacc[ds][4 * g + 0] * inv_l,
                                      oacc[ds][4 * g + 1] * inv_l);
      const unsigned w1 = cvt_pk_bf16(oacc[ds][4 * g + 2] * inv_l,
                                      oacc[ds][4 * g + 3] * inv_l);
      uint2 wv;
      wv.x = w0;
      wv.y = w1;
      *reinterpret_cast<uint2*>(orow + d0) = wv;
    }
  }
  if (hi == 0)
    lse[((long)b * n_heads + h) * S + qrow] =
        m_run * 0.6931471805599453f + __logf(l_run);
}
#undef V6_GLDS_K
#undef V6_LOAD_V
#undef V6_WRITE_V

// ===========================================================================
// v7 forward: v6's math with a 3-deep ALL-glds staging pipeline.
//
// v6 parks ~49% of wave cycles at waits/barriers: its __syncthreads()
// carries a vmcnt(0) drain (glds in flight) and the V register staging
// serializes a global-load wait into the middle of every tile. v7:
//   * K AND row-major V arrive by glds into a 3-slot ring (issue runs two
//     tiles ahead; nothing in the main loop ever waits vmcnt(0));
//   * the transposed V image is built LDS->LDS (2 b128 reads + 8 paired
//     b32 writes per thread) from the landed row image — no global
//     staging registers at all;
//   * barriers are RAW s_barrier (guide: "3-buffer glds + raw barrier,
//     counted vmcnt only"), one per tile, at tile end, guarding ring
//     reuse and publishing the next transposed image. The transpose
//     itself needs no barrier: every wave stages by glds exactly the
//     rows it transposes, so its own counted vmcnt covers them.
//
// MASK (also on the dq/dv/dk kernels): ATTN_MASK_CAUSAL is the causal
// kernel, tiles up to the diagonal, mask on the diagonal band.
// ATTN_MASK_NONE compiles the bound, the tile skip and the mask out: every q
// block visits all S_kv/64 kv tiles, for the blocks of ring attention that
// lie wholly below the diagonal. Those may be rectangular: the non-causal
// kernels take the q length S and the k/v length S_kv apart, the others never
// read S_kv (S_q == S_kv == S). ATTN_MASK_DOC is the causal kernel under a
// per-token document mask (below). Pipeline, ring depth, waits and barriers
// are shared.
// ===========================================================================

#define ATTN_MASK_NONE 0
#define ATTN_MASK_CAUSAL 1
#define ATTN_MASK_DOC 2

// ===========================================================================
// Document-masked causal attention: the ATTN_MASK_DOC instantiations of the
// v7 forward and the dq/dv/dk kernels. bounds, the last kernel argument
// (nullptr and never read in the other two modes), is int32 [2, B, S]:
// bounds[0,b,s] the window index of the first token of s's document (start),
// bounds[1,b,s] that of its last (end). q sees kv iff start[q] <= kv <= q,
// which for valid bounds (contiguous intervals, start and end constant on
// each) equals kv <= q <= end[kv]. The mask is shared by all heads.
//
// The text is the causal kernel's; the document lines sit under
// `if constexpr` and compile-time ternaries on MASK, so the other
// instantiations keep their instruction streams
// (profiles/r12_doc_merge.md). What the mode adds:
//   * fwd/dq: the lane owning q row qrow loads start once and masks
//     kvr < start next to kvr > qrow. The kv walk begins at the workgroup-
//     uniform tile attn_doc_tiles_q(start[b, qb*256], qb).first (ring sources,
//     slots and have2 count from there; the walk has at least 4 tiles, so the
//     prologue issues two unconditionally); a wave also sits out tiles wholly
//     before the smallest start of its 32 rows, and masks every tile that
//     some row's start cuts, not the diagonal band alone.
//   * dv/dk: the lane owning kv row kvrow loads end once and masks q > end
//     next to q < kvrow. The q walk stops at the workgroup-uniform tile
//     attn_doc_tiles_kv(end[b, last row of the block], kvb, S).last. Strip
//     ownership is the identity (256 neighbouring kv rows per workgroup) as a
//     compile-time fact, whatever `fold` says; the mode is instantiated
//     unsplit only, without workspace: q ranges differ per document, so
//     neither the fold nor the pair balances them (ROADMAP).
//
// Any int32 content is safe: a lane's start is clamped to [0, qrow], its end
// to [kvrow, S-1], and both tile ranges are clamped below, so every address
// derived from bounds stays inside the operands. Invalid bounds (not a
// partition) give wrong numbers, never an out-of-range access.
//
// Forward and fully masked tiles. A row can meet tiles in which all its
// entries are masked before its first real score: row 400 of a block whose
// row 256 belongs to an earlier document, in a strip that also holds rows of
// that document. Its masked scores are -1e30, so the first such tile sets
// m_run = -1e30 (alpha 0 from -inf) and P = exp2(-1e30 - -1e30) = 1 on the
// masked entries: l_run and oacc collect finite garbage. Further masked
// tiles keep m_run (pm - m_run = 0). The first tile with a real score x has
// x - m_run > 8, so the wave rescales, and alpha = exp2(-1e30 - x) is exactly
// 0: garbage * 0 = 0, and from there masked entries give exp2(-1e30 - m) = 0
// as in the causal kernel. That tile always comes because start <= qrow by
// the clamp: every row sees its own diagonal entry. The rescale decision is
// wave-wide (__all), so rows of two documents in one 32-row strip influence
// each other's rounding (not their masks); the backward has no such coupling.
// ===========================================================================

struct AttnTiles { int first, last; };       // inclusive 64-row tile range

__host__ __device__ __forceinline__ int attn_clampi(int x, int lo, int hi) {
  return x < lo ? lo : (x > hi ? hi : x);
}
// kv tiles q block qb (256 rows) walks when its first row's document starts
// at `start`: from that tile, at most the block's own first, to the diagonal
__host__ __device__ __forceinline__ AttnTiles attn_doc_tiles_q(int start,
                                                               int qb) {
  AttnTiles t;
  t.first = attn_clampi(start / 64, 0, qb * 4);
  t.last = qb * 4 + 3;
  return t;
}
// q tiles kv block kvb walks when its last row's document ends at `end`
__host__ __device__ __forceinline__ AttnTiles attn_doc_tiles_kv(int end,
                                                                int kvb,
                                                                int S) {
  AttnTiles t;
  t.first = kvb * 4;
  t.last = attn_clampi(end / 64 + 1, kvb * 4 + 1, S / 64) - 1;
  return t;
}

// smallest and largest of a per-row value over the wave's 32 rows (lanes
// low and low + 32 hold the same row), as wave-uniform scalars
__device__ __forceinline__ void attn_wave_minmax(int x, int& lo, int& hi_) {
  int mn = x, mx = x;
#pragma unroll
  for (int off = 1; off < 32; off <<= 1) {
    mn = min(mn, __shfl_xor(mn, off, 64));
    mx = max(mx, __shfl_xor(mx, off, 64));
  }
  lo = __builtin_amdgcn_readfirstlane(mn);
  hi_ = __builtin_amdgcn_readfirstlane(mx);
}

// One kv tile of the v7 forward for one wave: S = K Q^T (2 x 32x32 MFMA
// accumulators), scale and mask, online softmax with the lazy (> 8) rescale,
// P repacked to bf16, O += V^T P. One text for attn_fwd_v7_kernel<MASK> and
// attn_prefill_paged_kernel; a macro, not a function, because passing qf,
// oacc, m_run and l_run by reference moved every caller's stream
// (profiles/r14_paged_fold.md). It reads the names in scope where it is
// used: kb, vtb (this tile's K rows and transposed V), kv0, active,
// need_mask, qf, qrow, low, hi, scale2, DOC, start, and updates oacc, m_run,
// l_run. Without documents DOC is false and start 0. Documents (see the v7
// header): a row whose tiles so far were all masked sits at m_run = -1e30
// and is rescaled by exactly 0 at its first real one.
#define ATTN_V7_TILE()                                                      \
  f32x16 s0, s1;                                                            \
  AttnFrag pa[4];                                                           \
  float pm = -INFINITY;                                                     \
  if (active) {                                                             \
    _Pragma("unroll")                                                       \
    for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }              \
    _Pragma("unroll")                                                       \
    for (int kc = 0; kc < 8; ++kc) {                                        \
      bf16x8 a0 = *reinterpret_cast<const bf16x8*>(                         \
          &kb[k_byte(low, kc * 16 + hi * 8)]);                              \
      s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                         \
          a0, qf[kc].v, s0, 0, 0, 0);                                       \
      bf16x8 a1 = *reinterpret_cast<const bf16x8*>(                         \
          &kb[k_byte(32 + low, kc * 16 + hi * 8)]);                         \
      s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                         \
          a1, qf[kc].v, s1, 0, 0, 0);                                       \
    }                                                                       \
    if (need_mask) {                                                        \
      _Pragma("unroll")                                                     \
      for (int r = 0; r < 16; ++r) {                                        \
        const int kvr = kv0 + (r & 3) + 8 * (r >> 2) + 4 * hi;              \
        float x0 = s0[r] * scale2;                                          \
        if (kvr > qrow || (DOC && kvr < start)) x0 = -1e30f;                \
        s0[r] = x0;                                                         \
        float x1 = s1[r] * scale2;                                          \
        if (kvr + 32 > qrow || (DOC && kvr + 32 < start)) x1 = -1e30f;      \
        s1[r] = x1;                                                         \
        pm = fmaxf(pm, fmaxf(x0, x1));                                      \
      }                                                                     \
    } else {                                                                \
      _Pragma("unroll")                                                     \
      for (int r = 0; r < 16; ++r) {                                        \
        s0[r] *= scale2;                                                    \
        s1[r] *= scale2;                                                    \
        pm = fmaxf(pm, fmaxf(s0[r], s1[r]));                                \
      }                                                                     \
    }                                                                       \
    pm = fmaxf(pm, __shfl_xor(pm, 32, 64));                                 \
    if (!__all(pm - m_run <= 8.0f)) {                                       \
      const float mn = fmaxf(m_run, pm);                                    \
      const float alpha = (m_run == -INFINITY)                              \
          ? 0.f : exp2_raw(m_run - mn);                                     \
      m_run = mn;                                                           \
      l_run *= alpha;                                                       \
      _Pragma("unroll")                                                     \
      for (int ds = 0; ds < 4; ++ds)                                        \
        _Pragma("unroll")                                                   \
        for (int r = 0; r < 16; ++r) oacc[ds][r] *= alpha;                  \
    }                                                                       \
    float psum = 0.f;                                                       \
    _Pragma("unroll")                                                       \
    for (int r = 0; r < 16; ++r) {                                          \
      const float p0 = exp2_raw(s0[r] - m_run);                             \
      const float p1 = exp2_raw(s1[r] - m_run);                             \
      s0[r] = p0;                                                           \
      s1[r] = p1;                                                           \
      psum += p0 + p1;                                                      \
    }                                                                       \
    psum += __shfl_xor(psum, 32, 64);                                       \
    l_run += psum;                                                          \
    _Pragma("unroll")                                                       \
    for (int sub = 0; sub < 2; ++sub) {                                     \
      _Pragma("unroll")                                                     \
      for (int cc = 0; cc < 2; ++cc) {                                      \
        pa[sub * 2 + cc].v = attn_repack(sub == 0 ? s0 : s1, cc * 8);       \
      }                                                                     \
    }                                                                       \
    _Pragma("unroll")                                                       \
    for (int c = 0; c < 4; ++c) {                                           \
      _Pragma("unroll")                                                     \
      for (int ds = 0; ds < 4; ++ds) {                                      \
        bf16x8 vf = *reinterpret_cast<const bf16x8*>(                       \
            &vtb[vt_byte(ds * 32 + low, c * 16 + hi * 8)]);                 \
        oacc[ds] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                 \
            vf, pa[c].v, oacc[ds], 0, 0, 0);                                \
      }                                                                     \
    }                                                                       \
  }

// the lane's share of one output row, O / l as bf16: 4 d per uint2 store
__device__ __forceinline__ void attn_v7_store_row(const f32x16 (&oacc)[4],
                                                  float inv_l, u16* orow,
                                                  int hi) {
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d0 = 8 * g + 4 * hi + 32 * ds;
      uint2 wv;
      wv.x = cvt_pk_bf16(oacc[ds][4 * g + 0] * inv_l,
                         oacc[ds][4 * g + 1] * inv_l);
      wv.y = cvt_pk_bf16(oacc[ds][4 * g + 2] * inv_l,
                         oacc[ds][4 * g + 3] * inv_l);
      *reinterpret_cast<uint2*>(orow + d0) = wv;
    }
  }
}

template <int MASK>
__global__ __launch_bounds__(512) void attn_fwd_v7_kernel(
    const u16* __restrict__ q, const u16* __restrict__ k,
    const u16* __restrict__ v, u16* __restrict__ out,
    float* __restrict__ lse,
    long q_sb, long q_sh, long q_ss,
    long k_sb, long k_sh, long k_ss,
    long v_sb, long v_sh, long v_ss,
    long o_sb, long o_sh, long o_ss,
    int n_heads, int gqa_group, int S, float scale2, int batch, int sched,
    int S_kv, const int* __restrict__ bounds) {
  // S is the q length: row blocks, qb, the lse row base. S_kv, the k/v
  // length of a rectangular block, is read by the non-causal kernel alone.
  constexpr bool CAUSAL = MASK != ATTN_MASK_NONE;   // documents are causal too
  constexpr bool DOC = MASK == ATTN_MASK_DOC;
  constexpr int NT = 512;
  const AttnBlock blk = attn_sched_block(blockIdx.x, S / 256, n_heads, batch,
                                         sched);
  const int qb = S / 256 - 1 - blk.rank;   // longest-running blocks first
  const int h = blk.head;
  const int b = blk.batch;
  const int hkv = h / gqa_group;
  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int low = lane & 31;
  const int hi = lane >> 5;

  // ring: K rows (swizzled image) + V rows (swizzled image), both glds;
  // 2 transposed-V images built locally
  __shared__ __attribute__((aligned(16))) u16 lds[ATTN_RING_U16];

  const int q0w = qb * 256 + wid * 32;
  const int qrow = q0w + low;

  // documents: this row's start, its extremes over the wave's rows, and the
  // first tile of the workgroup's walk; all 0 in the other modes
  int start = 0, smin = 0, smax = 0, t_begin = 0;
  if constexpr (DOC) {
    const int* startp = bounds + (long)b * S;
    start = attn_clampi(startp[qrow], 0, qrow);
    attn_wave_minmax(start, smin, smax);
    t_begin = attn_doc_tiles_q(startp[qb * 256], qb).first;
  }

  AttnFrag qf[8];
  attn_load_row(qf, q + (long)b * q_sb + (long)h * q_sh + (long)qrow * q_ss,
                hi);

  f32x16 oacc[4];
  attn_zero(oacc);
  float m_run = -INFINITY, l_run = 0.f;

  // causal: tiles up to the diagonal (documents: from t_begin, at least 4);
  // non-causal: every kv tile
  const int n_tiles = CAUSAL ? (qb + 1) * 4 - t_begin : S_kv / V6_BN;

  // glds source pointers (swizzle-inverted, advanced per issue)
  AttnRingSrc src = attn_ring_src(
      k + (long)b * k_sb + (long)hkv * k_sh + (long)t_begin * V6_BN * k_ss,
      k_ss,
      v + (long)b * v_sb + (long)hkv * v_sh + (long)t_begin * V6_BN * v_ss,
      v_ss, tid);

  // prologue: issue tiles 0 and 1; build Vt[0] once tile 0 lands (LDS->LDS
  // transpose of the landed V row image)
  attn_ring_issue(lds, 0, src);
  if (DOC || n_tiles > 1) attn_ring_issue(lds, 1, src);
  if (DOC || n_tiles > 1) v7_wait_vmcnt4(); else v7_wait_vmcnt0();
  v7_barrier();
  attn_transpose(attn_ring_v(lds, 0), attn_ring_t(lds, 0), tid);
  // tile 0's PV reads every wave's share of Vt[0] before the first in-loop
  // barrier (that one sits at the END of tile 0), so publish it here
  v7_barrier();

  for (int t = 0; t < n_tiles; ++t) {          // t counts from t_begin
    const int kv0 = (t_begin + t) * V6_BN;
    const bool have2 = (t + 2) < n_tiles;
    if (have2) attn_ring_issue(lds, (t + 2) % V7_RING, src);

    char* kb = reinterpret_cast<char*>(attn_ring_k(lds, t % V7_RING));
    char* vtb = attn_ring_t(lds, t & 1);
    // documents: also sit out tiles wholly before the wave's smallest start,
    // and mask every tile that some row's start cuts
    const bool active =
        !CAUSAL || (kv0 <= q0w + 31 && (!DOC || kv0 + V6_BN > smin));
    const bool need_mask =
        CAUSAL && (kv0 + V6_BN > q0w || (DOC && kv0 < smax));

    ATTN_V7_TILE()
    // end-of-tile: wait slot t+1 (counted — t+2 stays in flight), build
    // the NEXT transposed image (different Vt buffer than this tile's PV
    // reads, so it needs no pre-barrier), then ONE raw barrier guarding
    // ring reuse + Vt visibility for tile t+1
    if (t + 1 < n_tiles) {
      if (have2) v7_wait_vmcnt4(); else v7_wait_vmcnt0();
      attn_transpose(attn_ring_v(lds, (t + 1) % V7_RING),
                     attn_ring_t(lds, (t + 1) & 1), tid);
    }
    v7_barrier();
  }

  attn_v7_store_row(
      oacc, 1.0f / l_run,
      out + (long)b * o_sb + (long)h * o_sh + (long)qrow * o_ss, hi);
  if (hi == 0)
    lse[((long)b * n_heads + h) * S + qrow] =
        m_run * 0.6931471805599453f + __logf(l_run);
}

// ===========================================================================
// Paged prefill forward: the causal v7 forward with queries at arbitrary
// cache positions and K/V tiles found through a block table. A sibling of
// attn_fwd_v7_kernel built from the same pieces (attn_load_row, the ring,
// attn_transpose, ATTN_V7_TILE); its block source, ring issue, active /
// need_mask and epilogue guard are its own.
//
// q and out are packed rows [T, H, 128]; the pools are [n_pages, n_kv, 64,
// 128], table [B, max_pages] int32 as in the paged decode kernels. A cache
// page is 64 rows = one kv tile = one ring slot, and a kv head of a page is a
// contiguous [64, 128] slab: a lane's in-tile glds offset is constant
// (attn_glds_page_off) and only the wave-uniform slab base changes per tile.
//
// Grid n_blocks * H. Block i reads work[i] = (slot, q_row0, n_rows, pos0):
// rows q_row0 .. q_row0 + n_rows - 1 (n_rows <= 256) of q/out belong to
// block-table row `slot` and sit at cache positions pos0 .. pos0 + n_rows - 1
// (pos0 need not be a multiple of 64). Row r attends cache rows 0 .. pos0 + r;
// the walk is tiles 0 .. (pos0 + n_rows - 1) / 64. The stale rows of a last
// page lie beyond every position, so the causal mask covers them.
//
// The table entry of a tile is a wave-uniform scalar load, fetched one tile
// ahead of the issue that needs it (the entry for tile t + 3 during tile t),
// so no glds waits on a dependent scalar load.
//
// Rows beyond n_rows: such a lane carries the block's LAST valid row (same q,
// same position), takes part in every barrier and in the wave-wide rescale
// decision and stores nothing, so the output is a function of the valid
// inputs only. A wave without any valid row skips the MFMAs and keeps
// staging and the barriers.
//
// Every descriptor field is clamped before use (attn_prefill_clamp) and every
// table entry into [0, n_pages), so any int32 content of work and table is
// memory-safe; only valid content gives meaningful numbers. No lse is
// written. With the whole block at pos0 % 256 == 0 and n_rows == 256 the tile
// walk, the row-to-wave mapping, active/need_mask and the MFMA order are
// v7's: the output equals flash_attention_fwd_v7 on the gathered cache bit
// for bit.
//
// Garbage contract: cache rows beyond a row's position, and pages beyond the
// walk, may hold any FINITE values without changing a bit of the output
// (their scores are replaced by -1e30, P is exactly 0). NaN/Inf in unread V
// rows of a walked page is outside the contract: 0 * NaN in the PV MFMA.
// ===========================================================================

struct AttnPrefillBlock { int slot, q_row0, n_rows, pos0; };

// the clamps of one work row; T, B, max_pages >= 1 and max_pages * 64 fits
// an int (the launcher checks)
__host__ __device__ __forceinline__ AttnPrefillBlock attn_prefill_clamp(
    int slot, int q_row0, int n_rows, int pos0, int T, int B, int max_pages) {
  AttnPrefillBlock w;
  int cap = T < V6_BM ? T : V6_BM;
  if (max_pages * V6_BN < cap) cap = max_pages * V6_BN;
  w.slot = attn_clampi(slot, 0, B - 1);
  w.n_rows = attn_clampi(n_rows, 1, cap);
  w.q_row0 = attn_clampi(q_row0, 0, T - w.n_rows);
  w.pos0 = attn_clampi(pos0, 0, max_pages * V6_BN - w.n_rows);
  return w;
}

__global__ __launch_bounds__(512) void attn_prefill_paged_kernel(
    const u16* __restrict__ q, const u16* __restrict__ kpool,
    const u16* __restrict__ vpool, u16* __restrict__ out,
    const int* __restrict__ table, const int* __restrict__ work,
    int n_heads, int gqa_group, int n_kv, int T, int B, int n_pages,
    int max_pages, float scale2) {
  const int wi = blockIdx.x / n_heads;
  const int h = blockIdx.x - wi * n_heads;
  const int hkv = h / gqa_group;
  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int low = lane & 31;
  const int hi = lane >> 5;

  const int* wrow = work + (long)wi * 4;
  const AttnPrefillBlock w =
      attn_prefill_clamp(wrow[0], wrow[1], wrow[2], wrow[3], T, B, max_pages);

  __shared__ __attribute__((aligned(16))) u16 lds[ATTN_RING_U16];

  // the lane's row inside the block, held at the last valid one
  const int r0w = wid * 32;
  const bool wave_rows = r0w < w.n_rows;
  const int rr = r0w + low;
  const int reff = rr < w.n_rows ? rr : w.n_rows - 1;
  const int qrow = w.pos0 + reff;                    // cache position
  const int q0w = w.pos0 + r0w;                      // wave's first position
  const int qlastw = w.pos0 + (r0w + 31 < w.n_rows ? r0w + 31 : w.n_rows - 1);
  constexpr bool DOC = false;                        // ATTN_V7_TILE: causal
  const int start = 0;

  AttnFrag qf[8];
  attn_load_row(qf, q + ((long)(w.q_row0 + reff) * n_heads + h) * ATTN_D, hi);

  f32x16 oacc[4];
  attn_zero(oacc);
  float m_run = -INFINITY, l_run = 0.f;

  const int n_tiles = (w.pos0 + w.n_rows - 1) / V6_BN + 1;   // <= max_pages

  // lane-constant offsets inside a page slab; wave-uniform LDS base
  int goff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    goff[i] = attn_glds_page_off((tid & ~63) * 32 + i * 1024 + (tid & 63) * 16);
  const int lslot = (tid & ~63) * 16;
  const int* trow = table + (long)w.slot * max_pages;
  const long slab = (long)V6_BN * ATTN_D;

#define APF_PAGE(TT)                                                        \
  attn_clampi(trow[(TT) < max_pages ? (TT) : max_pages - 1], 0, n_pages - 1)
#define APF_ISSUE(SLOT, PAGE)                                               \
  {                                                                         \
    const long pb_ = ((long)(PAGE) * n_kv + hkv) * slab;                    \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                         \
      __builtin_amdgcn_global_load_lds(                                     \
          (const u32*)(kpool + pb_ + goff[i]),                              \
          (u32*)&attn_ring_k(lds, SLOT)[i * 512 + lslot], 16, 0, 0);        \
      __builtin_amdgcn_global_load_lds(                                     \
          (const u32*)(vpool + pb_ + goff[i]),                              \
          (u32*)&attn_ring_v(lds, SLOT)[i * 512 + lslot], 16, 0, 0);        \
    }                                                                       \
  }

  // prologue as v7's non-causal mode: n_tiles can be 1
  const int pg0 = APF_PAGE(0);
  const int pg1 = APF_PAGE(1);
  int pg_next = APF_PAGE(2);              // the entry the t = 0 issue needs
  APF_ISSUE(0, pg0);
  if (n_tiles > 1) APF_ISSUE(1, pg1);
  if (n_tiles > 1) v7_wait_vmcnt4(); else v7_wait_vmcnt0();
  v7_barrier();
  attn_transpose(attn_ring_v(lds, 0), attn_ring_t(lds, 0), tid);
  v7_barrier();

  for (int t = 0; t < n_tiles; ++t) {
    const int kv0 = t * V6_BN;
    const bool have2 = (t + 2) < n_tiles;
    if (have2) APF_ISSUE((t + 2) % V7_RING, pg_next);
    pg_next = APF_PAGE(t + 3);            // one tile ahead of its issue

    char* kb = reinterpret_cast<char*>(attn_ring_k(lds, t % V7_RING));
    char* vtb = attn_ring_t(lds, t & 1);
    const bool active = wave_rows && kv0 <= qlastw;
    const bool need_mask = kv0 + V6_BN > q0w;

    ATTN_V7_TILE()
    if (t + 1 < n_tiles) {
      if (have2) v7_wait_vmcnt4(); else v7_wait_vmcnt0();
      attn_transpose(attn_ring_v(lds, (t + 1) % V7_RING),
                     attn_ring_t(lds, (t + 1) & 1), tid);
    }
    v7_barrier();
  }
#undef APF_ISSUE
#undef APF_PAGE

  if (rr < w.n_rows)
    attn_v7_store_row(
        oacc, 1.0f / l_run,
        out + ((long)(w.q_row0 + rr) * n_heads + h) * ATTN_D, hi);
}

// ===========================================================================
// v6 flash-attention BACKWARD (causal, bf16, D=128, GQA).
//
// Standard flash backward split into two walks plus a delta precompute:
//   delta[q]   = rowsum(dO[q] * O[q])                       (attn_delta)
//   P          = exp2(S*scale*log2e - lse*log2e)            (recomputed)
//   dV[kv]    += P^T @ dO        dK[kv] += scale * dS^T @ Q (attn_bwd_dkdv)
//   dS         = P o (dP - delta),  dP = dO @ V^T
//   dQ[q]     += scale * dS @ K                             (attn_bwd_dq)
//
// No online softmax state (lse is known), so the backward is simpler per
// tile than the forward. Both kernels reuse the v6 layout machinery:
// operand-swapped 32x32x16 MFMAs keep the OWNED axis lane-local (q rows in
// dq, kv rows in dkdv), P/dS repack stays in registers via
// cvt_pk_bf16_f32 + permlane32_swap, row-major images use the k_byte
// swizzle, transposed images the vt_byte image. GQA: dq walks q heads;
// dkdv owns a kv head and loops the group's q heads, accumulating dK/dV
// in registers across the loop - or, SPLIT, owns one q head and leaves an
// fp32 partial for attn_bwd_reduce_kernel (see attn_bwd_use_split).
// ===========================================================================

__global__ __launch_bounds__(256) void attn_delta_kernel(
    const u16* __restrict__ dout, const u16* __restrict__ o,
    float* __restrict__ delta,
    long do_sb, long do_sh, long do_ss,
    long o_sb, long o_sh, long o_ss,
    int n_heads, int S) {
  // one 16-lane group per row; 8 elems per thread; grid (S/16, H, B)
  const int s = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int h = blockIdx.y;
  const int bi = blockIdx.z;
  if (s >= S) return;
  const long row = ((long)bi * n_heads + h) * S + s;   // delta is [B,H,S]
  const int e8 = (threadIdx.x & 15) * 8;
  union { uint4 u; u16 h[8]; } a, b;
  a.u = *reinterpret_cast<const uint4*>(
      dout + (long)bi * do_sb + (long)h * do_sh + (long)s * do_ss + e8);
  b.u = *reinterpret_cast<const uint4*>(
      o + (long)bi * o_sb + (long)h * o_sh + (long)s * o_ss + e8);
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    acc += bf2f_(a.h[j]) * bf2f_(b.h[j]);
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 15) == 0) delta[row] = acc;
}

// ---------------------------------------------------------------------------
// dQ kernel: one 512-thread WG owns 256 q rows (8 waves x 32, q lane-local).
// Per 64-kv tile: S^T = K@Q^T (16 MFMA), dP^T = V@dO^T (16), dS^T packed,
// dQ^T += K^T @ dS (16). LDS per buffer: K rows (k_byte) + K^T (vt image)
// + V rows (k_byte) = 50.4 KB, double-buffered.
// ---------------------------------------------------------------------------

#define BQ_K_U16 (V6_BN * ATTN_D)                      // K row image
#define BQ_KT_U16 (ATTN_D * (VT_PITCH_B / 2) + 128)    // K^T image
#define BQ_V_U16 (V6_BN * ATTN_D)                      // V row image
#define BQ_BUF_U16 (BQ_K_U16 + BQ_KT_U16 + BQ_V_U16)

template <int MASK>
__global__ __launch_bounds__(512) void attn_bwd_dq_kernel(
    const u16* __restrict__ q, const u16* __restrict__ k,
    const u16* __restrict__ v, const u16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    u16* __restrict__ dq,
    long q_sb, long q_sh, long q_ss,
    long k_sb, long k_sh, long k_ss,
    long v_sb, long v_sh, long v_ss,
    long do_sb, long do_sh, long do_ss,
    long dq_sb, long dq_sh, long dq_ss,
    int n_heads, int gqa_group, int S, float scale, int batch, int sched,
    int S_kv, const int* __restrict__ bounds) {
  // S: q length (row blocks, lse/delta row base); S_kv: k/v length, read by
  // the non-causal kernel alone; MASK, bounds and the document lines as in
  // attn_fwd_v7_kernel.
  // v7-style staging: K rows + V rows by glds into 3-slot rings, K^T
  // built LDS->LDS at tile end, ONE raw barrier per tile, counted vmcnt.
  constexpr bool CAUSAL = MASK != ATTN_MASK_NONE;
  constexpr bool DOC = MASK == ATTN_MASK_DOC;
  constexpr int NT = 512;
  const AttnBlock blk = attn_sched_block(blockIdx.x, S / 256, n_heads, batch,
                                         sched);
  const int qb = S / 256 - 1 - blk.rank;
  const int h = blk.head;
  const int b = blk.batch;
  const int hkv = h / gqa_group;
  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int low = lane & 31;
  const int hi = lane >> 5;
  const float scale2 = scale * ATTN_LOG2E;

  // the ring holds K and V rows; the transposed images are K^T
  __shared__ __attribute__((aligned(16))) u16 lds[ATTN_RING_U16];

  const int q0w = qb * 256 + wid * 32;
  const int qrow = q0w + low;

  int start = 0, smin = 0, smax = 0, t_begin = 0;
  if constexpr (DOC) {
    const int* startp = bounds + (long)b * S;
    start = attn_clampi(startp[qrow], 0, qrow);
    attn_wave_minmax(start, smin, smax);
    t_begin = attn_doc_tiles_q(startp[qb * 256], qb).first;
  }

  AttnFrag qf[8], dof[8];
  attn_load_row(qf, q + (long)b * q_sb + (long)h * q_sh + (long)qrow * q_ss,
                hi);
  attn_load_row(dof, dout + (long)b * do_sb + (long)h * do_sh
                         + (long)qrow * do_ss, hi);
  const long lrow = ((long)b * n_heads + h) * S + qrow;
  const float lse2 = lse[lrow] * ATTN_LOG2E;
  const float dlt = delta[lrow];

  f32x16 dqacc[4];
  attn_zero(dqacc);

  // causal: tiles up to the diagonal (documents: from t_begin, at least 4);
  // non-causal: every kv tile
  const int n_tiles = CAUSAL ? (qb + 1) * 4 - t_begin : S_kv / V6_BN;

  AttnRingSrc src = attn_ring_src(
      k + (long)b * k_sb + (long)hkv * k_sh + (long)t_begin * V6_BN * k_ss,
      k_ss,
      v + (long)b * v_sb + (long)hkv * v_sh + (long)t_begin * V6_BN * v_ss,
      v_ss, tid);

  attn_ring_issue(lds, 0, src);
  if (DOC || n_tiles > 1) attn_ring_issue(lds, 1, src);
  if (DOC || n_tiles > 1) v7_wait_vmcnt4(); else v7_wait_vmcnt0();
  v7_barrier();
  attn_transpose(attn_ring_k(lds, 0), attn_ring_t(lds, 0), tid);
  v7_barrier();   // tile 0 reads every wave's share of KT[0]

  for (int t = 0; t < n_tiles; ++t) {          // t counts from t_begin
    const int kv0 = (t_begin + t) * V6_BN;
    const bool have2 = (t + 2) < n_tiles;
    if (have2) attn_ring_issue(lds, (t + 2) % V7_RING, src);

    char* kb = reinterpret_cast<char*>(attn_ring_k(lds, t % V7_RING));
    char* vb = reinterpret_cast<char*>(attn_ring_v(lds, t % V7_RING));
    char* ktb = attn_ring_t(lds, t & 1);
    const bool active =
        !CAUSAL || (kv0 <= q0w + 31 && (!DOC || kv0 + V6_BN > smin));
    const bool need_mask =
        CAUSAL && (kv0 + V6_BN > q0w || (DOC && kv0 < smax));

    AttnFrag pds[4];
    if (active) {
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        f32x16 sx, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { sx[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) {
          bf16x8 a = *reinterpret_cast<const bf16x8*>(
              &kb[k_byte(sub * 32 + low, kc * 16 + hi * 8)]);
          sx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[kc].v, sx,
                                                       0, 0, 0);
          bf16x8 a2 = *reinterpret_cast<const bf16x8*>(
              &vb[k_byte(sub * 32 + low, kc * 16 + hi * 8)]);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, dof[kc].v, dp,
                                                       0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float x = sx[r] * scale2 - lse2;
          if (need_mask) {
            const int kvr = kv0 + sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (kvr > qrow || (DOC && kvr < start)) x = -1e30f;
          }
          const float p = exp2_raw(x);
          sx[r] = p * (dp[r] - dlt) * scale;
        }
#pragma unroll
        for (int cc = 0; cc < 2; ++cc)
          pds[sub * 2 + cc].v = attn_repack(sx, cc * 8);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) {
          bf16x8 kf = *reinterpret_cast<const bf16x8*>(
              &ktb[vt_byte(ds * 32 + low, c * 16 + hi * 8)]);
          dqacc[ds] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              kf, pds[c].v, dqacc[ds], 0, 0, 0);
        }
      }
    }
    if (t + 1 < n_tiles) {
      if (have2) v7_wait_vmcnt4(); else v7_wait_vmcnt0();
      attn_transpose(attn_ring_k(lds, (t + 1) % V7_RING),
                     attn_ring_t(lds, (t + 1) & 1), tid);
    }
    v7_barrier();
  }

  u16* dqrow = dq + (long)b * dq_sb + (long)h * dq_sh + (long)qrow * dq_ss;
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) attn_store_bf16(dqrow, dqacc[ds], ds, hi);
}

// ---------------------------------------------------------------------------
// dV kernel: one 512-thread WG owns 256 kv rows (8 waves x 32, kv
// lane-local); loops the GQA group's q heads and their q tiles.
//   S^T tile: C[q32][kv32] = Q @ K^T   (K fragments persistent in registers)
//   P = 2^(s*scale2 - lse2[q]) (masked on the diagonal band)
//   dV^T += dO^T @ P: C[d][kv] via A = dO^T image, B = P-fragment repack
// LDS per buffer: Q row image + dO^T image + lse tile.
// ---------------------------------------------------------------------------

#define BV_Q_U16 (V6_BN * ATTN_D)
#define BV_DOT_U16 (ATTN_D * (VT_PITCH_B / 2) + 128)
#define BV_LSE_U16 128                      // 64 f32
#define BV_BUF_U16 (BV_Q_U16 + BV_DOT_U16 + BV_LSE_U16)

// Staging of one q tile for the dV walks (attn_bwd_dv_kernel and
// attn_bwd_dv_pair_kernel): Q rows by glds, the two dO rows of the lane into
// dtst, the lse tile; then dtst into the transposed dO image. Macros over the
// names in scope (lds, qgp, dtp, dtst, qstep, dostep, lbase, wu64, tid,
// LSEOFF, DOTOFF): as shared functions they moved the stream of all four
// dv/dk kernels (profiles/r09_attention_refactor.md).
#define BV_STAGE_IN(BUFI, QT)                                               \
    {                                                                       \
      _Pragma("unroll")                                                     \
      for (int i = 0; i < 2; ++i) {                                         \
        __builtin_amdgcn_global_load_lds(                                   \
            (const u32*)qgp[i], (u32*)&lds[BUFI][(i * 512 + wu64 * 64) * 8],\
            16, 0, 0);                                                      \
        qgp[i] += qstep;                                                    \
      }                                                                     \
      dtst[0] = *reinterpret_cast<const uint4*>(dtp[0]);                    \
      dtst[1] = *reinterpret_cast<const uint4*>(dtp[1]);                    \
      dtp[0] += dostep;                                                     \
      dtp[1] += dostep;                                                     \
      if (tid < 64)                                                         \
        *reinterpret_cast<float*>(                                          \
            &lds[BUFI][LSEOFF / 2 + tid * 2]) =                             \
            lbase[(QT) * 64 + tid] * ATTN_LOG2E;                   \
    }
#define BV_WRITE_DOT(BUF)                                                   \
    {                                                                       \
      const int rp2_ = (tid >> 4) * 2;                                      \
      const int c8_ = (tid & 15) * 8;                                       \
      union { uint4 u4; u16 h[8]; } va_, vb_;                               \
      va_.u4 = dtst[0];                                                     \
      vb_.u4 = dtst[1];                                                     \
      _Pragma("unroll")                                                     \
      for (int j = 0; j < 8; ++j) {                                         \
        const u32 pair_ = (u32)va_.h[j] | ((u32)vb_.h[j] << 16);            \
        *reinterpret_cast<u32*>(&(BUF)[DOTOFF + vt_byte(c8_ + j, rp2_)]) =  \
            pair_;                                                          \
      }                                                                     \
    }

template <int MASK, bool SPLIT>
__global__ __launch_bounds__(512) void attn_bwd_dv_kernel(
    const u16* __restrict__ q, const u16* __restrict__ k,
    const u16* __restrict__ dout, const float* __restrict__ lse,
    u16* __restrict__ dv,
    long q_sb, long q_sh, long q_ss,
    long k_sb, long k_sh, long k_ss,
    long do_sb, long do_sh, long do_ss,
    long dv_sb, long dv_sh, long dv_ss,
    int n_heads, int n_kv_heads, int S, float scale,
    float* __restrict__ ws, int batch, int sched, int fold, int S_kv_nc,
    const int* __restrict__ bounds) {
  // MASK and bounds as in attn_fwd_v7_kernel; documents are unsplit, with
  // identity strips whatever `fold` holds.
  constexpr bool CAUSAL = MASK != ATTN_MASK_NONE;
  constexpr bool DOC = MASK == ATTN_MASK_DOC;
  static_assert(!(DOC && SPLIT), "the document mode is unsplit only");
  // S is the q length (q tiles, lse/delta row base). The kv length sets the
  // row blocks, the strips and the workspace rows; it is S on the causal
  // path, where the extra argument is never read.
  const int S_kv = CAUSAL ? S : S_kv_nc;
  // SPLIT: the workgroup owns (kv block, Q head, batch), walks that one
  // head and leaves its fp32 accumulator in ws [B,H,S,128];
  // attn_bwd_reduce_kernel sums the group's partials. Otherwise it owns
  // (kv block, kv head, batch) and loops the group's q heads.
  const AttnBlock blk = attn_sched_block(
      blockIdx.x, S_kv / 256, SPLIT ? n_heads : n_kv_heads, batch, sched);
  const int kvb = blk.rank;                  // kv block of 256 (asc = heavy 1st)
  const int gqa_group = n_heads / n_kv_heads;
  const int hkv = SPLIT ? blk.head / gqa_group : blk.head;
  const int b = blk.batch;
  const int g_lo = SPLIT ? blk.head - hkv * gqa_group : 0;
  const int g_hi = SPLIT ? g_lo + 1 : gqa_group;
  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int low = lane & 31;
  const int hi = lane >> 5;
  const float scale2 = scale * ATTN_LOG2E;

  __shared__ __attribute__((aligned(16))) u16 lds[2][BV_BUF_U16];
  char* lds0 = reinterpret_cast<char*>(&lds[0][0]);
  char* lds1 = reinterpret_cast<char*>(&lds[1][0]);
  const int DOTOFF = BV_Q_U16 * 2;
  const int LSEOFF = (BV_Q_U16 + BV_DOT_U16) * 2;

  // the non-causal walk is equal work already: identity whatever the flag
  const AttnStrips strips = attn_bwd_strips(
      MASK == ATTN_MASK_CAUSAL ? fold : ATTN_STRIPS_IDENTITY, kvb,
      __builtin_amdgcn_readfirstlane(wid), S_kv / 256);
  const int kv0w = strips.kv0w;
  const int kvrow = kv0w + low;              // this lane's kv row

  // documents: this kv row's end, its extremes over the wave's rows, and the
  // last q tile of the workgroup's walk (one past it, as qtn)
  int end = 0, emin = 0, emax = 0, qtn = S / 64;
  if constexpr (DOC) {
    const int* endp = bounds + ((long)batch + b) * S;
    end = attn_clampi(endp[kvrow], kvrow, S - 1);
    attn_wave_minmax(end, emin, emax);
    qtn = attn_doc_tiles_kv(endp[kvb * 256 + 255], kvb, S).last + 1;
  }

  // K row in registers (persistent across the whole WG lifetime)
  const u16* kptr = k + (long)b * k_sb + (long)hkv * k_sh + (long)kvrow * k_ss;
  AttnFrag kf[8];
#pragma unroll
  for (int kc = 0; kc < 8; ++kc)
    kf[kc].u = *reinterpret_cast<const uint4*>(kptr + kc * 16 + hi * 8);

  f32x16 dvacc[4];
  attn_zero(dvacc);

  const int qt0 = CAUSAL ? strips.qt0 : 0;   // first q tile that sees us
  const int wu64 = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint4 dtst[2];

  for (int g = g_lo; g < g_hi; ++g) {
    const int h = hkv * gqa_group + g;
    const u16* qbase = q + (long)b * q_sb + (long)h * q_sh;
    const u16* dobase = dout + (long)b * do_sb + (long)h * do_sh;
    const float* lbase = lse + ((long)b * n_heads + h) * S;

    // per-thread staging pointers for this head
    const u16* qgp[2];
    const u16* dtp[2];
    {
      const int idx0 = tid, idx1 = 512 + tid;
      const int L0 = idx0 * 16, L1 = idx1 * 16;
      const int r0 = L0 >> 8, r1 = L1 >> 8;
      const int in0 = (((L0 & 255) ^ ((r0 & 15) << 4)) >> 1);
      const int in1 = (((L1 & 255) ^ ((r1 & 15) << 4)) >> 1);
      qgp[0] = qbase + (long)(qt0 * 64 + r0) * q_ss + in0;
      qgp[1] = qbase + (long)(qt0 * 64 + r1) * q_ss + in1;
      const int rp2 = (tid >> 4) * 2;
      const int c8 = (tid & 15) * 8;
      dtp[0] = dobase + (long)(qt0 * 64 + rp2) * do_ss + c8;
      dtp[1] = dobase + (long)(qt0 * 64 + rp2 + 1) * do_ss + c8;
    }
    const long qstep = (long)64 * q_ss;
    const long dostep = (long)64 * do_ss;

    BV_STAGE_IN(0, qt0)
    BV_WRITE_DOT(lds0)
    __syncthreads();

    int cur = 0;
    for (int qt = qt0; qt < qtn; ++qt) {
      const bool have_next = (qt + 1) < qtn;
      if (have_next) BV_STAGE_IN(cur ^ 1, qt + 1)

      char* qb_ = cur ? lds1 : lds0;
      char* dob = qb_ + DOTOFF;
      const float* lse2t = reinterpret_cast<const float*>(qb_ + LSEOFF);
      // this wave's kv rows need q >= kv0w; skip tiles fully in the past
      // (documents: and those past the largest end of its rows)
      const bool active =
          !CAUSAL || (qt * 64 + 63 >= kv0w && (!DOC || qt * 64 <= emax));
      const bool need_mask =
          CAUSAL && (qt * 64 < kv0w + 32 || (DOC && qt * 64 + 63 > emin));

      AttnFrag pf[4];
      if (active) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          f32x16 s;
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
          for (int kc = 0; kc < 8; ++kc) {
            bf16x8 a = *reinterpret_cast<const bf16x8*>(
                &qb_[k_byte(sub * 32 + low, kc * 16 + hi * 8)]);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, kf[kc].v, s,
                                                        0, 0, 0);
          }
          // P = 2^(s*scale2 - lse2[q]); mask q < kv (documents: and q > end)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int qr = (r & 3) + 8 * (r >> 2) + 4 * hi;   // q within sub
            float x = s[r] * scale2 - lse2t[sub * 32 + qr];
            const int qa = qt * 64 + sub * 32 + qr;
            if (need_mask && (qa < kvrow || (DOC && qa > end))) x = -1e30f;
            s[r] = exp2_raw(x);
          }
          // repack P (C[q][kv]) -> B-fragments [k=q chunk][n=kv]
#pragma unroll
          for (int cc = 0; cc < 2; ++cc) {
            pf[sub * 2 + cc].v = attn_repack(s, cc * 8);
          }
        }
      }
      if (have_next) {
        char* nb = cur ? lds0 : lds1;
        BV_WRITE_DOT(nb)
      }
      if (active) {
        // dV^T += dO^T @ P over 4 q chunks x 4 d subtiles
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
          for (int ds = 0; ds < 4; ++ds) {
            bf16x8 af = *reinterpret_cast<const bf16x8*>(
                &dob[vt_byte(ds * 32 + low, c * 16 + hi * 8)]);
            dvacc[ds] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                af, pf[c].v, dvacc[ds], 0, 0, 0);
          }
        }
      }
      __syncthreads();
      cur ^= 1;
    }
  }

  if (SPLIT) {
    // fp32 partial of this q head: 4 consecutive d per accumulator quad
    float* wrow =
        ws + (((long)b * n_heads + blk.head) * S_kv + kvrow) * ATTN_D;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) attn_store_f32(wrow, dvacc[ds], ds, hi);
    return;
  }
  // epilogue: dv rows through (batch, kv head, row) strides
  u16* dvrow = dv + (long)b * dv_sb + (long)hkv * dv_sh + (long)kvrow * dv_ss;
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) attn_store_bf16(dvrow, dvacc[ds], ds, hi);
}

// ---------------------------------------------------------------------------
// dK kernel: same kv-block walk as dV.
//   S^T: C[q][kv] = Q @ K^T       (K fragments persistent)
//   dP:  C[q][kv] = dO @ V^T      (V fragments persistent)
//   dS = P o (dP - delta[q]) * scale
//   dK^T += Q^T @ dS: C[d][kv] via A = Q^T image, B = dS repack
// LDS per buffer: Q row image + dO row image + Q^T image + lse + delta.
// ---------------------------------------------------------------------------

#define BK_Q_U16 (V6_BN * ATTN_D)
#define BK_DO_U16 (V6_BN * ATTN_D)
#define BK_QT_U16 (ATTN_D * (VT_PITCH_B / 2) + 128)
#define BK_LSE_U16 128
#define BK_DLT_U16 128
#define BK_BUF_U16 (BK_Q_U16 + BK_DO_U16 + BK_QT_U16 + BK_LSE_U16 + BK_DLT_U16)

// Staging of one q tile for the dK walks (attn_bwd_dk_kernel and
// attn_bwd_dk_pair_kernel): Q and dO rows by glds, the two Q rows of the lane
// into qtst, the lse and delta tiles; then qtst into the transposed Q image.
// Macros over the names in scope, as BV_STAGE_IN.
#define BK_STAGE_IN(BUFI, QT)                                               \
    {                                                                       \
      _Pragma("unroll")                                                     \
      for (int i = 0; i < 2; ++i) {                                         \
        __builtin_amdgcn_global_load_lds(                                   \
            (const u32*)qgp[i], (u32*)&lds[BUFI][(i * 512 + wu64 * 64) * 8],\
            16, 0, 0);                                                      \
        qgp[i] += qstep;                                                    \
        __builtin_amdgcn_global_load_lds(                                   \
            (const u32*)dgp[i],                                             \
            (u32*)&lds[BUFI][DOOFF / 2 + (i * 512 + wu64 * 64) * 8],        \
            16, 0, 0);                                                      \
        dgp[i] += dostep;                                                   \
      }                                                                     \
      qtst[0] = *reinterpret_cast<const uint4*>(qtp[0]);                    \
      qtst[1] = *reinterpret_cast<const uint4*>(qtp[1]);                    \
      qtp[0] += qstep;                                                      \
      qtp[1] += qstep;                                                      \
      if (tid < 64)                                                         \
        *reinterpret_cast<float*>(&lds[BUFI][LSEOFF / 2 + tid * 2]) =       \
            lbase[(QT) * 64 + tid] * ATTN_LOG2E;                   \
      else if (tid < 128)                                                   \
        *reinterpret_cast<float*>(                                          \
            &lds[BUFI][DLTOFF / 2 + (tid - 64) * 2]) =                      \
            dbase[(QT) * 64 + tid - 64];                                    \
    }
#define BK_WRITE_QT(BUF)                                                    \
    {                                                                       \
      const int rp2_ = (tid >> 4) * 2;                                      \
      const int c8_ = (tid & 15) * 8;                                       \
      union { uint4 u4; u16 h[8]; } va_, vb_;                               \
      va_.u4 = qtst[0];                                                     \
      vb_.u4 = qtst[1];                                                     \
      _Pragma("unroll")                                                     \
      for (int j = 0; j < 8; ++j) {                                         \
        const u32 pair_ = (u32)va_.h[j] | ((u32)vb_.h[j] << 16);            \
        *reinterpret_cast<u32*>(&(BUF)[QTOFF + vt_byte(c8_ + j, rp2_)]) =   \
            pair_;                                                          \
      }                                                                     \
    }

template <int MASK, bool SPLIT>
__global__ __launch_bounds__(512) void attn_bwd_dk_kernel(
    const u16* __restrict__ q, const u16* __restrict__ k,
    const u16* __restrict__ v, const u16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    u16* __restrict__ dk,
    long q_sb, long q_sh, long q_ss,
    long k_sb, long k_sh, long k_ss,
    long v_sb, long v_sh, long v_ss,
    long do_sb, long do_sh, long do_ss,
    long dk_sb, long dk_sh, long dk_ss,
    int n_heads, int n_kv_heads, int S, float scale,
    float* __restrict__ ws, int batch, int sched, int fold, int S_kv_nc,
    const int* __restrict__ bounds) {
  constexpr bool CAUSAL = MASK != ATTN_MASK_NONE;            // see dv
  constexpr bool DOC = MASK == ATTN_MASK_DOC;
  static_assert(!(DOC && SPLIT), "the document mode is unsplit only");
  // S is the q length (q tiles, lse/delta row base). The kv length sets the
  // row blocks, the strips and the workspace rows; it is S on the causal
  // path, where the extra argument is never read.
  const int S_kv = CAUSAL ? S : S_kv_nc;
  const AttnBlock blk = attn_sched_block(
      blockIdx.x, S_kv / 256, SPLIT ? n_heads : n_kv_heads, batch, sched);
  const int kvb = blk.rank;
  const int gqa_group = n_heads / n_kv_heads;
  const int hkv = SPLIT ? blk.head / gqa_group : blk.head;   // see dv
  const int b = blk.batch;
  const int g_lo = SPLIT ? blk.head - hkv * gqa_group : 0;
  const int g_hi = SPLIT ? g_lo + 1 : gqa_group;
  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int low = lane & 31;
  const int hi = lane >> 5;
  const float scale2 = scale * ATTN_LOG2E;

  __shared__ __attribute__((aligned(16))) u16 lds[2][BK_BUF_U16];
  char* lds0 = reinterpret_cast<char*>(&lds[0][0]);
  char* lds1 = reinterpret_cast<char*>(&lds[1][0]);
  const int DOOFF = BK_Q_U16 * 2;
  const int QTOFF = (BK_Q_U16 + BK_DO_U16) * 2;
  const int LSEOFF = (BK_Q_U16 + BK_DO_U16 + BK_QT_U16) * 2;
  const int DLTOFF = LSEOFF + BK_LSE_U16 * 2;

  const AttnStrips strips = attn_bwd_strips(
      MASK == ATTN_MASK_CAUSAL ? fold : ATTN_STRIPS_IDENTITY, kvb,
      __builtin_amdgcn_readfirstlane(wid), S_kv / 256);   // see dv
  const int kv0w = strips.kv0w;
  const int kvrow = kv0w + low;

  int end = 0, emin = 0, emax = 0, qtn = S / 64;            // see dv
  if constexpr (DOC) {
    const int* endp = bounds + ((long)batch + b) * S;
    end = attn_clampi(endp[kvrow], kvrow, S - 1);
    attn_wave_minmax(end, emin, emax);
    qtn = attn_doc_tiles_kv(endp[kvb * 256 + 255], kvb, S).last + 1;
  }

  const u16* kptr = k + (long)b * k_sb + (long)hkv * k_sh + (long)kvrow * k_ss;
  const u16* vptr = v + (long)b * v_sb + (long)hkv * v_sh + (long)kvrow * v_ss;
  AttnFrag kf[8], vf[8];
#pragma unroll
  for (int kc = 0; kc < 8; ++kc) {
    kf[kc].u = *reinterpret_cast<const uint4*>(kptr + kc * 16 + hi * 8);
    vf[kc].u = *reinterpret_cast<const uint4*>(vptr + kc * 16 + hi * 8);
  }

  f32x16 dkacc[4];
  attn_zero(dkacc);

  const int qt0 = CAUSAL ? strips.qt0 : 0;
  const int wu64 = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint4 qtst[2];

  for (int g = g_lo; g < g_hi; ++g) {
    const int h = hkv * gqa_group + g;
    const u16* qbase = q + (long)b * q_sb + (long)h * q_sh;
    const u16* dobase = dout + (long)b * do_sb + (long)h * do_sh;
    const float* lbase = lse + ((long)b * n_heads + h) * S;
    const float* dbase = delta + ((long)b * n_heads + h) * S;

    const u16* qgp[2];
    const u16* dgp[2];
    const u16* qtp[2];
    {
      const int idx0 = tid, idx1 = 512 + tid;
      const int L0 = idx0 * 16, L1 = idx1 * 16;
      const int r0 = L0 >> 8, r1 = L1 >> 8;
      const int in0 = (((L0 & 255) ^ ((r0 & 15) << 4)) >> 1);
      const int in1 = (((L1 & 255) ^ ((r1 & 15) << 4)) >> 1);
      qgp[0] = qbase + (long)(qt0 * 64 + r0) * q_ss + in0;
      qgp[1] = qbase + (long)(qt0 * 64 + r1) * q_ss + in1;
      dgp[0] = dobase + (long)(qt0 * 64 + r0) * do_ss + in0;
      dgp[1] = dobase + (long)(qt0 * 64 + r1) * do_ss + in1;
      const int rp2 = (tid >> 4) * 2;
      const int c8 = (tid & 15) * 8;
      qtp[0] = qbase + (long)(qt0 * 64 + rp2) * q_ss + c8;
      qtp[1] = qbase + (long)(qt0 * 64 + rp2 + 1) * q_ss + c8;
    }
    const long qstep = (long)64 * q_ss;
    const long dostep = (long)64 * do_ss;

    BK_STAGE_IN(0, qt0)
    BK_WRITE_QT(lds0)
    __syncthreads();

    int cur = 0;
    for (int qt = qt0; qt < qtn; ++qt) {
      const bool have_next = (qt + 1) < qtn;
      if (have_next) BK_STAGE_IN(cur ^ 1, qt + 1)

      char* qb_ = cur ? lds1 : lds0;
      char* dob = qb_ + DOOFF;
      char* qtb = qb_ + QTOFF;
      const float* lse2t = reinterpret_cast<const float*>(qb_ + LSEOFF);
      const float* dltt = reinterpret_cast<const float*>(qb_ + DLTOFF);
      const bool active =
          !CAUSAL || (qt * 64 + 63 >= kv0w && (!DOC || qt * 64 <= emax));
      const bool need_mask =
          CAUSAL && (qt * 64 < kv0w + 32 || (DOC && qt * 64 + 63 > emin));

      AttnFrag pf[4];
      if (active) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          f32x16 s, dp;
#pragma unroll
          for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
          for (int kc = 0; kc < 8; ++kc) {
            bf16x8 a = *reinterpret_cast<const bf16x8*>(
                &qb_[k_byte(sub * 32 + low, kc * 16 + hi * 8)]);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, kf[kc].v, s,
                                                        0, 0, 0);
            bf16x8 a2 = *reinterpret_cast<const bf16x8*>(
                &dob[k_byte(sub * 32 + low, kc * 16 + hi * 8)]);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, vf[kc].v, dp,
                                                         0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int qr = (r & 3) + 8 * (r >> 2) + 4 * hi;
            float x = s[r] * scale2 - lse2t[sub * 32 + qr];
            const int qa = qt * 64 + sub * 32 + qr;
            if (need_mask && (qa < kvrow || (DOC && qa > end))) x = -1e30f;
            const float p = exp2_raw(x);
            s[r] = p * (dp[r] - dltt[sub * 32 + qr]) * scale;
          }
#pragma unroll
          for (int cc = 0; cc < 2; ++cc) {
            pf[sub * 2 + cc].v = attn_repack(s, cc * 8);
          }
        }
      }
      if (have_next) {
        char* nb = cur ? lds0 : lds1;
        BK_WRITE_QT(nb)
      }
      if (active) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
          for (int ds = 0; ds < 4; ++ds) {
            bf16x8 af = *reinterpret_cast<const bf16x8*>(
                &qtb[vt_byte(ds * 32 + low, c * 16 + hi * 8)]);
            dkacc[ds] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                af, pf[c].v, dkacc[ds], 0, 0, 0);
          }
        }
      }
      __syncthreads();
      cur ^= 1;
    }
  }

  if (SPLIT) {
    // fp32 partial of this q head: 4 consecutive d per accumulator quad
    float* wrow =
        ws + (((long)b * n_heads + blk.head) * S_kv + kvrow) * ATTN_D;
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) attn_store_f32(wrow, dkacc[ds], ds, hi);
    return;
  }
  u16* dkrow = dk + (long)b * dk_sb + (long)hkv * dk_sh + (long)kvrow * dk_ss;
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) attn_store_bf16(dkrow, dkacc[ds], ds, hi);
}

// ---------------------------------------------------------------------------
// dV and dK with PAIR ownership (attn_bwd_pair): causal, unsplit. Same grid,
// staging and element arithmetic as the causal unsplit attn_bwd_dv_kernel and
// attn_bwd_dk_kernel; what differs is who computes what.
//
// Barriers: every wave reaches, per phase and q head, one barrier after the
// first staging and two per tile (after the fragment exchange writes, and
// the end-of-tile one), all outside `if (active)`; qt0, qtn and the head
// range are workgroup-uniform, so the count is equal for the eight waves
// on every path, the last tile (no have_next) and the phase change
// included. Partners share kv0w, hence `active`, so the exchange is skipped
// by both or by neither. A wave rewrites its exchange chunks only after the
// end-of-tile barrier that follows its partner's read of them.
//
// The A operand of d subtile ds0 + j sits ds0 * 32 rows further into the
// transposed image: vt_byte(ds0 * 32 + d, kv) == ds0 * 32 * VT_PITCH_B +
// vt_byte(d, kv) for ds0 in {0, 2}, because 64 * VT_PITCH_B = 9 * 1024
// leaves the XORed slot bits alone and the key of m + 8 is the key of m.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(512) void attn_bwd_dv_pair_kernel(
    const u16* __restrict__ q, const u16* __restrict__ k,
    const u16* __restrict__ dout, const float* __restrict__ lse,
    u16* __restrict__ dv,
    long q_sb, long q_sh, long q_ss,
    long k_sb, long k_sh, long k_ss,
    long do_sb, long do_sh, long do_ss,
    long dv_sb, long dv_sh, long dv_ss,
    int n_heads, int n_kv_heads, int S, float scale, int batch, int sched) {
  const int nrb = S / 256;
  const AttnBlock blk = attn_sched_block(blockIdx.x, nrb, n_kv_heads, batch,
                                         sched);
  const int gqa_group = n_heads / n_kv_heads;
  const int hkv = blk.head;
  const int b = blk.batch;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int low = lane & 31;
  const int hi = lane >> 5;
  const float scale2 = scale * ATTN_LOG2E;

  __shared__ __attribute__((aligned(16))) u16 lds[2][BV_BUF_U16];
  __shared__ __attribute__((aligned(16))) uint4 xch[ATTN_PAIR_XCH_U4];
  char* lds0 = reinterpret_cast<char*>(&lds[0][0]);
  char* lds1 = reinterpret_cast<char*>(&lds[1][0]);
  const int DOTOFF = BV_Q_U16 * 2;
  const int LSEOFF = (BV_Q_U16 + BV_DOT_U16) * 2;

  const int qtn = S / 64;
  const int wu64 = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint4 dtst[2];

#pragma unroll 1
  for (int phase = 0; phase < 2; ++phase) {
    const AttnPair pr = attn_bwd_pair(blk.rank, phase, wu64, nrb);
    const int kv0w = pr.kv0w;
    const int kvrow = kv0w + low;            // this lane's kv row
    const int sub = pr.sub;
    const int aoff = pr.ds0 * 32 * VT_PITCH_B;

    const u16* kptr =
        k + (long)b * k_sb + (long)hkv * k_sh + (long)kvrow * k_ss;
    AttnFrag kf[8];
#pragma unroll
    for (int kc = 0; kc < 8; ++kc)
      kf[kc].u = *reinterpret_cast<const uint4*>(kptr + kc * 16 + hi * 8);

    f32x16 dvacc[2];
  attn_zero(dvacc);

    const int qt0 = pr.qt0;

    for (int g = 0; g < gqa_group; ++g) {
      const int h = hkv * gqa_group + g;
      const u16* qbase = q + (long)b * q_sb + (long)h * q_sh;
      const u16* dobase = dout + (long)b * do_sb + (long)h * do_sh;
      const float* lbase = lse + ((long)b * n_heads + h) * S;

      const u16* qgp[2];
      const u16* dtp[2];
      {
        const int idx0 = tid, idx1 = 512 + tid;
        const int L0 = idx0 * 16, L1 = idx1 * 16;
        const int r0 = L0 >> 8, r1 = L1 >> 8;
        const int in0 = (((L0 & 255) ^ ((r0 & 15) << 4)) >> 1);
        const int in1 = (((L1 & 255) ^ ((r1 & 15) << 4)) >> 1);
        qgp[0] = qbase + (long)(qt0 * 64 + r0) * q_ss + in0;
        qgp[1] = qbase + (long)(qt0 * 64 + r1) * q_ss + in1;
        const int rp2 = (tid >> 4) * 2;
        const int c8 = (tid & 15) * 8;
        dtp[0] = dobase + (long)(qt0 * 64 + rp2) * do_ss + c8;
        dtp[1] = dobase + (long)(qt0 * 64 + rp2 + 1) * do_ss + c8;
      }
      const long qstep = (long)64 * q_ss;
      const long dostep = (long)64 * do_ss;

      BV_STAGE_IN(0, qt0)
      BV_WRITE_DOT(lds0)
      __syncthreads();

      int cur = 0;
      for (int qt = qt0; qt < qtn; ++qt) {
        const bool have_next = (qt + 1) < qtn;
        if (have_next) BV_STAGE_IN(cur ^ 1, qt + 1)

        char* qb_ = cur ? lds1 : lds0;
        char* dob = qb_ + DOTOFF;
        const float* lse2t = reinterpret_cast<const float*>(qb_ + LSEOFF);
        const bool active = qt * 64 + 63 >= kv0w;
        const bool need_mask = qt * 64 < kv0w + 32;

        AttnFrag pf[4];
        if (active) {
          f32x16 s;
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
          for (int kc = 0; kc < 8; ++kc) {
            bf16x8 a = *reinterpret_cast<const bf16x8*>(
                &qb_[k_byte(sub * 32 + low, kc * 16 + hi * 8)]);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, kf[kc].v, s,
                                                        0, 0, 0);
          }
          // P = 2^(s*scale2 - lse2[q]); mask q < kv
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int qr = (r & 3) + 8 * (r >> 2) + 4 * hi;   // q within sub
            float x = s[r] * scale2 - lse2t[sub * 32 + qr];
            if (need_mask && qt * 64 + sub * 32 + qr < kvrow) x = -1e30f;
            s[r] = exp2_raw(x);
          }
          // repack P (C[q][kv]) -> B-fragments [k=q chunk][n=kv], chunks
          // 2*sub and 2*sub + 1, into the exchange area
#pragma unroll
          for (int cc = 0; cc < 2; ++cc) {
            AttnFrag f;
            f.v = attn_repack(s, cc * 8);
            xch[attn_pair_xch(wu64, sub * 2 + cc) + lane] = f.u;
          }
        }
        v7_barrier();                        // fragments of both subs written
        if (active) {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            pf[c].u = xch[attn_pair_xch(wu64, c) + lane];
        }
        if (have_next) {
          char* nb = cur ? lds0 : lds1;
          BV_WRITE_DOT(nb)
        }
        if (active) {
          // dV^T += dO^T @ P over 4 q chunks x this wave's 2 d subtiles
#pragma unroll
          for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              bf16x8 af = *reinterpret_cast<const bf16x8*>(
                  &dob[aoff + vt_byte(j * 32 + low, c * 16 + hi * 8)]);
              dvacc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                  af, pf[c].v, dvacc[j], 0, 0, 0);
            }
          }
        }
        __syncthreads();
        cur ^= 1;
      }
    }

    // this wave's two d subtiles of the strip's rows
    u16* dvrow =
        dv + (long)b * dv_sb + (long)hkv * dv_sh + (long)kvrow * dv_ss;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = 8 * g + 4 * hi + 32 * (pr.ds0 + j);
        const unsigned w0 = cvt_pk_bf16(dvacc[j][4 * g + 0],
                                        dvacc[j][4 * g + 1]);
        const unsigned w1 = cvt_pk_bf16(dvacc[j][4 * g + 2],
                                        dvacc[j][4 * g + 3]);
        uint2 wv;
        wv.x = w0;
        wv.y = w1;
        *reinterpret_cast<uint2*>(dvrow + d0) = wv;
      }
    }
  }
}

__global__ __launch_bounds__(512) void attn_bwd_dk_pair_kernel(
    const u16* __restrict__ q, const u16* __restrict__ k,
    const u16* __restrict__ v, const u16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    u16* __restrict__ dk,
    long q_sb, long q_sh, long q_ss,
    long k_sb, long k_sh, long k_ss,
    long v_sb, long v_sh, long v_ss,
    long do_sb, long do_sh, long do_ss,
    long dk_sb, long dk_sh, long dk_ss,
    int n_heads, int n_kv_heads, int S, float scale, int batch, int sched) {
  const int nrb = S / 256;
  const AttnBlock blk = attn_sched_block(blockIdx.x, nrb, n_kv_heads, batch,
                                         sched);
  const int gqa_group = n_heads / n_kv_heads;
  const int hkv = blk.head;
  const int b = blk.batch;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int low = lane & 31;
  const int hi = lane >> 5;
  const float scale2 = scale * ATTN_LOG2E;

  __shared__ __attribute__((aligned(16))) u16 lds[2][BK_BUF_U16];
  __shared__ __attribute__((aligned(16))) uint4 xch[ATTN_PAIR_XCH_U4];
  char* lds0 = reinterpret_cast<char*>(&lds[0][0]);
  char* lds1 = reinterpret_cast<char*>(&lds[1][0]);
  const int DOOFF = BK_Q_U16 * 2;
  const int QTOFF = (BK_Q_U16 + BK_DO_U16) * 2;
  const int LSEOFF = (BK_Q_U16 + BK_DO_U16 + BK_QT_U16) * 2;
  const int DLTOFF = LSEOFF + BK_LSE_U16 * 2;

  const int qtn = S / 64;
  const int wu64 = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint4 qtst[2];

#pragma unroll 1
  for (int phase = 0; phase < 2; ++phase) {
    const AttnPair pr = attn_bwd_pair(blk.rank, phase, wu64, nrb);
    const int kv0w = pr.kv0w;
    const int kvrow = kv0w + low;
    const int sub = pr.sub;
    const int aoff = pr.ds0 * 32 * VT_PITCH_B;

    const u16* kptr =
        k + (long)b * k_sb + (long)hkv * k_sh + (long)kvrow * k_ss;
    const u16* vptr =
        v + (long)b * v_sb + (long)hkv * v_sh + (long)kvrow * v_ss;
    AttnFrag kf[8], vf[8];
#pragma unroll
    for (int kc = 0; kc < 8; ++kc) {
      kf[kc].u = *reinterpret_cast<const uint4*>(kptr + kc * 16 + hi * 8);
      vf[kc].u = *reinterpret_cast<const uint4*>(vptr + kc * 16 + hi * 8);
    }

    f32x16 dkacc[2];
  attn_zero(dkacc);

    const int qt0 = pr.qt0;

    for (int g = 0; g < gqa_group; ++g) {
      const int h = hkv * gqa_group + g;
      const u16* qbase = q + (long)b * q_sb + (long)h * q_sh;
      const u16* dobase = dout + (long)b * do_sb + (long)h * do_sh;
      const float* lbase = lse + ((long)b * n_heads + h) * S;
      const float* dbase = delta + ((long)b * n_heads + h) * S;

      const u16* qgp[2];
      const u16* dgp[2];
      const u16* qtp[2];
      {
        const int idx0 = tid, idx1 = 512 + tid;
        const int L0 = idx0 * 16, L1 = idx1 * 16;
        const int r0 = L0 >> 8, r1 = L1 >> 8;
        const int in0 = (((L0 & 255) ^ ((r0 & 15) << 4)) >> 1);
        const int in1 = (((L1 & 255) ^ ((r1 & 15) << 4)) >> 1);
        qgp[0] = qbase + (long)(qt0 * 64 + r0) * q_ss + in0;
        qgp[1] = qbase + (long)(qt0 * 64 + r1) * q_ss + in1;
        dgp[0] = dobase + (long)(qt0 * 64 + r0) * do_ss + in0;
        dgp[1] = dobase + (long)(qt0 * 64 + r1) * do_ss + in1;
        const int rp2 = (tid >> 4) * 2;
        const int c8 = (tid & 15) * 8;
        qtp[0] = qbase + (long)(qt0 * 64 + rp2) * q_ss + c8;
        qtp[1] = qbase + (long)(qt0 * 64 + rp2 + 1) * q_ss + c8;
      }
      const long qstep = (long)64 * q_ss;
      const long dostep = (long)64 * do_ss;

      BK_STAGE_IN(0, qt0)
      BK_WRITE_QT(lds0)
      __syncthreads();

      int cur = 0;
      for (int qt = qt0; qt < qtn; ++qt) {
        const bool have_next = (qt + 1) < qtn;
        if (have_next) BK_STAGE_IN(cur ^ 1, qt + 1)

        char* qb_ = cur ? lds1 : lds0;
        char* dob = qb_ + DOOFF;
        char* qtb = qb_ + QTOFF;
        const float* lse2t = reinterpret_cast<const float*>(qb_ + LSEOFF);
        const float* dltt = reinterpret_cast<const float*>(qb_ + DLTOFF);
        const bool active = qt * 64 + 63 >= kv0w;
        const bool need_mask = qt * 64 < kv0w + 32;

        AttnFrag pf[4];
        if (active) {
          f32x16 s, dp;
#pragma unroll
          for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
          for (int kc = 0; kc < 8; ++kc) {
            bf16x8 a = *reinterpret_cast<const bf16x8*>(
                &qb_[k_byte(sub * 32 + low, kc * 16 + hi * 8)]);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, kf[kc].v, s,
                                                        0, 0, 0);
            bf16x8 a2 = *reinterpret_cast<const bf16x8*>(
                &dob[k_byte(sub * 32 + low, kc * 16 + hi * 8)]);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, vf[kc].v, dp,
                                                         0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int qr = (r & 3) + 8 * (r >> 2) + 4 * hi;
            float x = s[r] * scale2 - lse2t[sub * 32 + qr];
            if (need_mask && qt * 64 + sub * 32 + qr < kvrow) x = -1e30f;
            const float p = exp2_raw(x);
            s[r] = p * (dp[r] - dltt[sub * 32 + qr]) * scale;
          }
#pragma unroll
          for (int cc = 0; cc < 2; ++cc) {
            AttnFrag f;
            f.v = attn_repack(s, cc * 8);
            xch[attn_pair_xch(wu64, sub * 2 + cc) + lane] = f.u;
          }
        }
        v7_barrier();                        // fragments of both subs written
        if (active) {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            pf[c].u = xch[attn_pair_xch(wu64, c) + lane];
        }
        if (have_next) {
          char* nb = cur ? lds0 : lds1;
          BK_WRITE_QT(nb)
        }
        if (active) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              bf16x8 af = *reinterpret_cast<const bf16x8*>(
                  &qtb[aoff + vt_byte(j * 32 + low, c * 16 + hi * 8)]);
              dkacc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                  af, pf[c].v, dkacc[j], 0, 0, 0);
            }
          }
        }
        __syncthreads();
        cur ^= 1;
      }
    }

    u16* dkrow =
        dk + (long)b * dk_sb + (long)hkv * dk_sh + (long)kvrow * dk_ss;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = 8 * g + 4 * hi + 32 * (pr.ds0 + j);
        const unsigned w0 = cvt_pk_bf16(dkacc[j][4 * g + 0],
                                        dkacc[j][4 * g + 1]);
        const unsigned w1 = cvt_pk_bf16(dkacc[j][4 * g + 2],
                                        dkacc[j][4 * g + 3]);
        uint2 wv;
        wv.x = w0;
        wv.y = w1;
        *reinterpret_cast<uint2*>(dkrow + d0) = wv;
      }
    }
  }
}
#undef BV_STAGE_IN
#undef BV_WRITE_DOT
#undef BK_STAGE_IN
#undef BK_WRITE_QT

// ---------------------------------------------------------------------------
// Split dK/dV: sum the gqa_group fp32 partials of each kv head in fixed
// order ((p0 + p1) + p2) + ..., round once to bf16 (the same
// v_cvt_pk_bf16_f32 the unsplit epilogue uses) and write dk and dv through
// their strides. One 16-lane group per (batch, kv head, row), 8 elements
// per lane; blockIdx.y picks dk (0) or dv (1). No atomics: bit-reproducible.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void attn_bwd_reduce_kernel(
    const float* __restrict__ ws_k, const float* __restrict__ ws_v,
    u16* __restrict__ dk, u16* __restrict__ dv,
    long dk_sb, long dk_sh, long dk_ss,
    long dv_sb, long dv_sh, long dv_ss,
    int n_heads, int n_kv_heads, int S, long n_rows) {
  const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (row >= n_rows) return;
  const int sub = threadIdx.x & 15;
  const int gqa_group = n_heads / n_kv_heads;
  const long bh = row / S;                    // b * n_kv_heads + hkv
  const int s = (int)(row - bh * S);
  const long bi = bh / n_kv_heads;
  const int hkv = (int)(bh - bi * n_kv_heads);
  const bool is_v = blockIdx.y != 0;
  const float* src = (is_v ? ws_v : ws_k)
      + ((bi * n_heads + (long)hkv * gqa_group) * S + s) * ATTN_D + sub * 8;
  const long hstep = (long)S * ATTN_D;
  float4 a0 = reinterpret_cast<const float4*>(src)[0];
  float4 a1 = reinterpret_cast<const float4*>(src)[1];
  for (int g = 1; g < gqa_group; ++g) {
    const float4 p0 = reinterpret_cast<const float4*>(src + g * hstep)[0];
    const float4 p1 = reinterpret_cast<const float4*>(src + g * hstep)[1];
    a0.x += p0.x; a0.y += p0.y; a0.z += p0.z; a0.w += p0.w;
    a1.x += p1.x; a1.y += p1.y; a1.z += p1.z; a1.w += p1.w;
  }
  uint4 o;
  o.x = cvt_pk_bf16(a0.x, a0.y);
  o.y = cvt_pk_bf16(a0.z, a0.w);
  o.z = cvt_pk_bf16(a1.x, a1.y);
  o.w = cvt_pk_bf16(a1.z, a1.w);
  u16* dst = is_v
      ? dv + bi * dv_sb + (long)hkv * dv_sh + (long)s * dv_ss
      : dk + bi * dk_sb + (long)hkv * dk_sh + (long)s * dk_ss;
  *reinterpret_cast<uint4*>(dst + sub * 8) = o;
}

// ---------------------------------------------------------------------------
// attn_merge: fold one block result (o_blk bf16, lse_blk) into the running
// fp32 accumulator (o_acc, lse_acc), in place:
//   lse_new = logaddexp(lse_acc, lse_blk)
//   o_acc   = o_acc * exp(lse_acc - lse_new) + o_blk * exp(lse_blk - lse_new)
// One 16-lane group per row, 8 elements per lane (one 16-B bf16 load, two
// 16-B fp32 loads and stores). The group's lane 0 alone reads and writes
// the row's lse pair and hands the two weights to the other 15 lanes. The
// weights go through the pair's max, so an accumulator at (0, -inf) takes
// weight exactly 0 and the block weight exactly 1 (no -inf - -inf).
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void attn_merge_kernel(
    float* __restrict__ o_acc, float* __restrict__ lse_acc,
    const u16* __restrict__ o_blk, const float* __restrict__ lse_blk,
    long ob_sb, long ob_sh, long ob_ss, int n_heads, int S, long n_rows) {
  const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (row >= n_rows) return;          // whole 16-lane groups leave together
  const int sub = threadIdx.x & 15;
  float wa = 0.f, wb = 0.f;
  if (sub == 0) {
    const float la = lse_acc[row], lb = lse_blk[row];
    const float m = fmaxf(la, lb);
    if (m != -INFINITY) {
      const float ea = __expf(la - m), eb = __expf(lb - m);
      const float sum = ea + eb;
      wa = ea / sum;
      wb = eb / sum;
      lse_acc[row] = m + __logf(sum);
    }
  }
  wa = __shfl(wa, 0, 16);
  wb = __shfl(wb, 0, 16);
  const long bh = row / S;
  const int s = (int)(row - bh * S);
  const long bi = bh / n_heads;
  const int h = (int)(bh - bi * n_heads);
  union { uint4 u; u16 h[8]; } ob;
  ob.u = *reinterpret_cast<const uint4*>(
      o_blk + bi * ob_sb + (long)h * ob_sh + (long)s * ob_ss + sub * 8);
  float4* acc = reinterpret_cast<float4*>(o_acc + row * ATTN_D + sub * 8);
  float4 a0 = acc[0], a1 = acc[1];
  a0.x = a0.x * wa + bf2f_(ob.h[0]) * wb;
  a0.y = a0.y * wa + bf2f_(ob.h[1]) * wb;
  a0.z = a0.z * wa + bf2f_(ob.h[2]) * wb;
  a0.w = a0.w * wa + bf2f_(ob.h[3]) * wb;
  a1.x = a1.x * wa + bf2f_(ob.h[4]) * wb;
  a1.y = a1.y * wa + bf2f_(ob.h[5]) * wb;
  a1.z = a1.z * wa + bf2f_(ob.h[6]) * wb;
  a1.w = a1.w * wa + bf2f_(ob.h[7]) * wb;
  acc[0] = a0;
  acc[1] = a1;
}

// batch / head / row strides of one [B, heads, S, 128] operand (elements)
struct AttnStride { long sb, sh, ss; };
// the three strides as consecutive kernel arguments
#define ATTN_S3(s) (s).sb, (s).sh, (s).ss

static inline AttnStride attn_dense_stride(int n_heads, int S) {
  return {(long)n_heads * S * ATTN_D, (long)S * ATTN_D, (long)ATTN_D};
}

// triple i of the host long[] the *_strided and block entries take
static inline AttnStride attn_stride_at(const long* st, int i) {
  return {st[3 * i], st[3 * i + 1], st[3 * i + 2]};
}

// The kernels move 16-byte vectors along D, so every stride must keep rows
// 16-byte aligned (a multiple of 8 bf16 elements).
static inline bool attn_strides_ok(const long* st, int n) {
  for (int i = 0; i < n; ++i)
    if (st[i] < 0 || st[i] % 8 != 0) return false;
  return true;
}

// Schedule of one launch. AITJ_ATTN_SCHED=legacy|balanced forces every
// kernel to that decode (read on every call, so both can be timed
// alternately in one process); unset or anything else takes the default.
static int attn_sched_mode() {
  const char* e = std::getenv("AITJ_ATTN_SCHED");
  if (e && std::strcmp(e, "legacy") == 0) return ATTN_SCHED_LEGACY;
  return ATTN_SCHED_BALANCED;
}

// Host-callable decode (tests/test_attention_sched_cpu.py). sched: 0 legacy,
// 1 balanced. Returns nonzero for an id outside the grid.
extern "C" int attn_sched_decode(int sched, int id, int n_row_blocks,
                                 int n_heads, int batch, int* rank,
                                 int* head, int* b) {
  if (n_row_blocks <= 0 || n_heads <= 0 || batch <= 0 || id < 0 ||
      (long)id >= (long)n_row_blocks * n_heads * batch ||
      (sched != ATTN_SCHED_LEGACY && sched != ATTN_SCHED_BALANCED))
    return -1;
  const AttnBlock blk = attn_sched_block((unsigned)id, (unsigned)n_row_blocks,
                                         (unsigned)n_heads, (unsigned)batch,
                                         sched);
  *rank = blk.rank;
  *head = blk.head;
  *b = blk.batch;
  return 0;
}

// 1-D grid of the four scheduled kernels; the launchers refuse shapes
// whose workgroup count does not fit an int
static inline bool attn_grid_ok(int S, int n_heads, int batch) {
  return (long)(S / 256) * n_heads * batch <= 0x7fffffffL;
}

// v7 launch shared by attn_fwd, attn_fwd_v7 (contiguous [B,H,S,D] out) and
// attn_fwd_strided (out through batch/head/row strides)
static int launch_fwd_v7(void* stream, const void* q, const void* k,
                          const void* v, void* out, void* lse,
                          AttnStride qs, AttnStride ks, AttnStride vs,
                          AttnStride os, int batch, int n_heads,
                          int n_kv_heads, int S, float scale,
                          bool causal = true, int S_kv = 0) {
  // S_kv: k/v rows of a rectangular non-causal block; 0 = square
  if (S_kv == 0) S_kv = S;
  if (!attn_grid_ok(S, n_heads, batch) || (causal && S_kv != S)) return -1;
  const float scale2 = scale * ATTN_LOG2E;   // fold log2(e)
  dim3 grid((S / 256) * n_heads * batch), block(512);
  hipLaunchKernelGGL(causal ? attn_fwd_v7_kernel<ATTN_MASK_CAUSAL>
                            : attn_fwd_v7_kernel<ATTN_MASK_NONE>, grid, block, 0,
                     reinterpret_cast<hipStream_t>(stream),
                     (const u16*)q, (const u16*)k, (const u16*)v,
                     (u16*)out, (float*)lse, ATTN_S3(qs), ATTN_S3(ks),
                     ATTN_S3(vs), ATTN_S3(os), n_heads,
                     n_heads / n_kv_heads, S, scale2, batch,
                     attn_sched_mode(), S_kv, (const int*)nullptr);
  return 0;
}

extern "C" int attn_fwd(void* stream, const void* q, const void* k,
                        const void* v, void* out, void* lse,
                        long q_sb, long q_sh, long q_ss,
                        long k_sb, long k_sh, long k_ss,
                        long v_sb, long v_sh, long v_ss,
                        int batch, int n_heads, int n_kv_heads, int S,
                        float scale) {
  if (S <= 0 || n_heads <= 0 || batch <= 0 || n_kv_heads <= 0 ||
      n_heads % n_kv_heads != 0)
    return -1;
  if (S % 128 == 0) {
    // BM=256 preferred: halves the K/V staging traffic vs BM=128 (each kv
    // tile is read by half as many workgroups); measured 344 vs 587 us at
    // B1H32S4096. BM=128 covers the S%128 shapes.
    const float scale2 = scale * ATTN_LOG2E;   // fold log2(e)
    if (S % 256 == 0) {
      // v7: 3-deep all-glds pipeline, single raw barrier per tile
      // (299 us vs v6's 346 at B1H32S4096; aotriton 425)
      return launch_fwd_v7(stream, q, k, v, out, lse, {q_sb, q_sh, q_ss},
                           {k_sb, k_sh, k_ss}, {v_sb, v_sh, v_ss},
                           attn_dense_stride(n_heads, S), batch, n_heads,
                           n_kv_heads, S, scale);
    }
    dim3 grid(S / 128, n_heads, batch), block(256);
    hipLaunchKernelGGL((attn_fwd_v6_kernel<4>), grid, block, 0,
                       reinterpret_cast<hipStream_t>(stream),
                       (const u16*)q, (const u16*)k, (const u16*)v, (u16*)out,
                       (float*)lse, q_sb, q_sh, q_ss, k_sb, k_sh, k_ss,
                       v_sb, v_sh, v_ss, n_heads, n_heads / n_kv_heads, S,
                       scale2);
    return 0;
  }
  if (S % ATTN_BM != 0 || n_kv_heads != n_heads) return -1;  // v5: no GQA
  dim3 grid(S / ATTN_BM, n_heads, batch), block(256);
  hipLaunchKernelGGL(attn_fwd_kernel, grid, block, 0,
                     reinterpret_cast<hipStream_t>(stream),
                     (const u16*)q, (const u16*)k, (const u16*)v, (u16*)out,
                     (float*)lse, q_sb, q_sh, q_ss, k_sb, k_sh, k_ss,
                     v_sb, v_sh, v_ss, n_heads, S, scale);
  return 0;
}

// 8-wave instantiation kept callable for A/B benchmarking
extern "C" int attn_fwd_nw8(void* stream, const void* q, const void* k,
                            const void* v, void* out, void* lse,
                            long q_sb, long q_sh, long q_ss,
                            long k_sb, long k_sh, long k_ss,
                            long v_sb, long v_sh, long v_ss,
                            int batch, int n_heads, int n_kv_heads, int S,
                            float scale) {
  if (S <= 0 || S % 256 != 0 || n_heads % n_kv_heads != 0) return -1;
  dim3 grid(S / 256, n_heads, batch), block(512);
  const float scale2 = scale * ATTN_LOG2E;
  hipLaunchKernelGGL((attn_fwd_v6_kernel<8>), grid, block, 0,
                     reinterpret_cast<hipStream_t>(stream),
                     (const u16*)q, (const u16*)k, (const u16*)v, (u16*)out,
                     (float*)lse, q_sb, q_sh, q_ss, k_sb, k_sh, k_ss,
                     v_sb, v_sh, v_ss, n_heads, n_heads / n_kv_heads, S,
                     scale2);
  return 0;
}

// v5 kept callable for A/B benchmarking (scripts/attnbench.py v5)
extern "C" int attn_fwd_v5(void* stream, const void* q, const void* k,
                           const void* v, void* out, void* lse,
                           long q_sb, long q_sh, long q_ss,
                           long k_sb, long k_sh, long k_ss,
                           long v_sb, long v_sh, long v_ss,
                           int batch, int n_heads, int S, float scale) {
  if (S <= 0 || S % ATTN_BM != 0 || n_heads <= 0 || batch <= 0) return -1;
  dim3 grid(S / ATTN_BM, n_heads, batch), block(256);
  hipLaunchKernelGGL(attn_fwd_kernel, grid, block, 0,
                     reinterpret_cast<hipStream_t>(stream),
                     (const u16*)q, (const u16*)k, (const u16*)v, (u16*)out,
                     (float*)lse, q_sb, q_sh, q_ss, k_sb, k_sh, k_ss,
                     v_sb, v_sh, v_ss, n_heads, S, scale);
  return 0;
}

// paged prefill forward (attn_prefill_paged_kernel): q/out [T, H, 128] bf16
// packed rows, pools [n_pages, n_kv, 64, 128] bf16 contiguous, block_table
// [B, max_pages] int32, work [n_blocks, 4] int32 device rows (slot, q_row0,
// n_rows, pos0), heaviest blocks first.
extern "C" int attn_prefill_paged(void* stream, const void* q,
                                  const void* k_pool, const void* v_pool,
                                  void* out, const void* block_table,
                                  const void* work, int n_blocks, int T,
                                  int n_heads, int n_kv_heads, int B,
                                  int n_pages, int max_pages, float scale) {
  if (n_blocks <= 0 || T <= 0 || n_heads <= 0 || n_kv_heads <= 0 ||
      n_heads % n_kv_heads != 0 || B <= 0 || n_pages <= 0 ||
      max_pages <= 0 || max_pages > (1 << 24) || !block_table || !work ||
      (long)n_blocks * n_heads > 0x7fffffffL)
    return -1;
  dim3 grid((unsigned)(n_blocks * n_heads)), block(512);
  hipLaunchKernelGGL(attn_prefill_paged_kernel, grid, block, 0,
                     reinterpret_cast<hipStream_t>(stream), (const u16*)q,
                     (const u16*)k_pool, (const u16*)v_pool, (u16*)out,
                     (const int*)block_table, (const int*)work, n_heads,
                     n_heads / n_kv_heads, n_kv_heads, T, B, n_pages,
                     max_pages, scale * ATTN_LOG2E);
  return 0;
}

// Host-callable clamp of one work row (tests/test_paged_prefill_cpu.py):
// io = (slot, q_row0, n_rows, pos0) in, the values the kernel uses out.
extern "C" int attn_prefill_work_decode(int* io, int T, int B,
                                        int max_pages) {
  if (!io || T <= 0 || B <= 0 || max_pages <= 0 || max_pages > (1 << 24))
    return -1;
  const AttnPrefillBlock w =
      attn_prefill_clamp(io[0], io[1], io[2], io[3], T, B, max_pages);
  io[0] = w.slot;
  io[1] = w.q_row0;
  io[2] = w.n_rows;
  io[3] = w.pos0;
  return 0;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

// delta[q] = rowsum(dO[q] * O[q]); delta is always dense [B,H,S] fp32
static void launch_delta(hipStream_t st, const void* out, const void* dout,
                         void* delta, AttnStride os, AttnStride dos,
                         int batch, int n_heads, int S) {
  hipLaunchKernelGGL(attn_delta_kernel, dim3(S / 16, n_heads, batch),
                     dim3(256), 0, st,
                     (const u16*)dout, (const u16*)out, (float*)delta,
                     ATTN_S3(dos), ATTN_S3(os), n_heads, S);
}

static inline bool attn_block_shape_ok(int batch, int n_heads,
                                       int n_kv_heads, int S) {
  return S > 0 && S % 256 == 0 && n_heads > 0 && batch > 0 &&
         n_kv_heads > 0 && n_heads % n_kv_heads == 0 &&
         attn_grid_ok(S, n_heads, batch);
}

// Whether dv/dk run split per q head. The one place that decides; read on
// every call. AITJ_ATTN_BWD_SPLIT: 0 or unset = never, 1 = always, auto =
// the measured rule below.
//
// Unset means unsplit because the split changes the fp32 association of the
// sum over a kv head's q heads: a few thousand of 8.4M dk/dv values per
// layer pass land one bf16 step away, and a training step does not
// reproduce the unsplit run's loss and weights bit for bit (Llama-3-8B,
// 5 steps: loss 12.462067 against 12.529497). Whoever turns it on chooses
// that; the default computes exactly what the unsplit kernels compute.
//
// auto: at 229-256 VGPRs a CU holds one 512-thread dv/dk workgroup, and an
// unsplit causal workgroup walks gqa_group * (n - kvb) units, the heaviest
// 1.9x the mean, so the grid only balances by backfill when it holds more
// than one workgroup per CU. Splitting multiplies the workgroup count by
// gqa_group at the price of 2 * B*H*S*128 fp32 written and read once.
// Measured at H=32 HKV=8 S=4096, dv + dk (+ reduction), us, unsplit ->
// split (profiles/r05_attention_balance.md):
//   causal      0.5 wg/CU (B=1) 1384 ->  554    1 wg/CU (B=2) 1568 -> 1085
//               2 wg/CU   (B=4) 1977 -> 2180    4 wg/CU (B=8) 3722 -> 4459
//   non-causal  0.5 wg/CU (B=1) 1387 ->  876    1 wg/CU (B=2) 1526 -> 1686
// So auto splits when the group has more than one head and the unsplit grid
// has fewer than 2 workgroups per CU (causal) or fewer than one
// (non-causal: equal work, splitting only helps to fill idle CUs).
// Re-measured with the unsplit walk folded (attn_bwd_use_fold): B=1 1147
// against 491 split, B=2 1203 against 921, B=4 1662 (unfolded) against
// 1892; the rule stands.
#define ATTN_NUM_CUS 256     // MI355X
static bool attn_bwd_use_split(int batch, int n_heads, int n_kv_heads, int S,
                               bool causal) {
  const char* e = std::getenv("AITJ_ATTN_BWD_SPLIT");
  if (e && std::strcmp(e, "1") == 0) return true;
  if (!e || std::strcmp(e, "auto") != 0) return false;
  if (n_heads == n_kv_heads) return false;
  const long wgs = (long)batch * n_kv_heads * (S / 256);
  return wgs < (long)(causal ? 2 : 1) * ATTN_NUM_CUS;
}

// Which ownership the causal dv/dk workgroups take: identity, folded strips
// (attn_bwd_strips) or pairs (attn_bwd_pair), per kernel. The one place
// that decides; read on every call. AITJ_ATTN_BWD_FOLD: 0 = identity, 1 =
// fold (causal), 2 = pair (causal and unsplit; a split launch takes the
// rule below instead); unset or anything else = the measured rule below.
// Neither fold nor pair changes a bit of dk or dv, so unlike the split the
// default may use them. Non-causal launches never fold or pair: equal work
// already.
//
// The fold evens out the work of the waves inside one workgroup; a
// workgroup still walks 4n - 2*rank tile steps per head, the longest as
// long as the identity's, and gains only where a SIMD runs one active wave
// instead of two (a tile step then takes 1/1.27 of the time in dv, 1/1.13
// in dk). With more than one workgroup per CU the identity's heavy-first
// order already balances by backfill, and the fold, which makes every
// workgroup long, loses. Measured at H=32 HKV=8 S=4096 causal, dv + dk
// (+ reduction), us, fold off -> on (profiles/r06_dkdv_fold.md):
//   unsplit  0.5 wg/CU (B=1) 1336 -> 1147    1 wg/CU (B=2) 1426 -> 1203
//            2 wg/CU   (B=4) 1662 -> 2066    4 wg/CU (B=8) 3372 -> 4439
//   split    2 wg/CU   (B=1)  491 ->  576    4 wg/CU (B=2)  921 -> 1136
//            8 wg/CU   (B=4) 1892 -> 2446   16 wg/CU (B=8) 4235 -> 5369
// So the rule folds when the dv/dk grid has at most one workgroup per CU.
// Between 1 and 2 per CU nothing was measured.
//
// The pair (the partners of a SIMD share one strip, every workgroup walks
// 4n + 2 steps with both waves busy) is a long workgroup like the fold's
// and loses to the identity's backfill in the same places. Unsplit, us,
// identity / fold / pair, two runs averaged
// (profiles/r08_dkdv_pair.md):
//   dv  B=1  521 /  417 /  425    B=2  568 /  438 /  445
//       B=4  691 /  803 /  963    B=8 1384 / 1748 / 2004
//   dk  B=1  808 /  726 /  588    B=2  862 /  774 /  620
//       B=4 1039 / 1310 / 1284    B=8 2099 / 2720 / 2661
// dk pairs where it folded before (at most one workgroup per CU): -19 to -20 %.
// dv does not: its tile step has too little MFMA work (8 + 8 per wave) to
// carry the second barrier, and the pair reads 7 us behind the fold there
// and 11 us behind it in the step trace. So unset gives dk the pair and dv
// the fold.
#define ATTN_BWD_DV 0
#define ATTN_BWD_DK 1
static int attn_bwd_use_fold(int batch, int n_heads, int n_kv_heads, int S,
                             bool causal, bool split, int kernel) {
  if (!causal) return ATTN_STRIPS_IDENTITY;
  const char* e = std::getenv("AITJ_ATTN_BWD_FOLD");
  if (e && std::strcmp(e, "0") == 0) return ATTN_STRIPS_IDENTITY;
  if (e && std::strcmp(e, "1") == 0) return ATTN_STRIPS_FOLD;
  if (e && std::strcmp(e, "2") == 0 && !split) return ATTN_STRIPS_PAIR;
  const long wgs = (long)batch * (split ? n_heads : n_kv_heads) * (S / 256);
  if (wgs > ATTN_NUM_CUS) return ATTN_STRIPS_IDENTITY;
  if (split || kernel != ATTN_BWD_DK) return ATTN_STRIPS_FOLD;
  return ATTN_STRIPS_PAIR;
}

// The ownership a launch of this shape gets right now (0 identity, 1 fold,
// 2 pair), for kernel 0 = dv, 1 = dk. Host only.
extern "C" int attn_bwd_fold_mode(int batch, int n_heads, int n_kv_heads,
                                  int S, int causal, int split, int kernel) {
  return attn_bwd_use_fold(batch, n_heads, n_kv_heads, S, causal != 0,
                           split != 0, kernel);
}

// Host-callable pair ownership (tests/test_attention_pair_cpu.py): workgroup
// rank, phase 0 (heavy half-block) or 1 (light), wave, row blocks -> the
// wave's first kv row, the phase's first q tile, the 32-row sub of each tile
// the wave computes, the half-open range [ds0, ds1) of d subtiles it
// accumulates, and the wave whose exchange chunks it reads. Returns nonzero
// for arguments outside the launch.
extern "C" int attn_bwd_pair_decode(int rank, int phase, int wid,
                                    int n_row_blocks, int* kv0w, int* qt0,
                                    int* sub, int* ds0, int* ds1, int* peer) {
  if (n_row_blocks <= 0 || rank < 0 || rank >= n_row_blocks || wid < 0 ||
      wid >= 8 || phase < 0 || phase > 1)
    return -1;
  const AttnPair p = attn_bwd_pair(rank, phase, wid, n_row_blocks);
  *kv0w = p.kv0w;
  *qt0 = p.qt0;
  *sub = p.sub;
  *ds0 = p.ds0;
  *ds1 = p.ds0 + 2;
  *peer = p.peer;
  return 0;
}

// Host-callable strip ownership (tests/test_attention_fold_cpu.py). fold: 0
// identity, 1 fold. Returns nonzero for arguments outside the launch.
extern "C" int attn_bwd_strips_decode(int fold, int rank, int wid,
                                      int n_row_blocks, int* kv0w, int* qt0) {
  if (n_row_blocks <= 0 || rank < 0 || rank >= n_row_blocks || wid < 0 ||
      wid >= 8 || (fold != ATTN_STRIPS_IDENTITY && fold != ATTN_STRIPS_FOLD))
    return -1;
  const AttnStrips s = attn_bwd_strips(fold, rank, wid, n_row_blocks);
  *kv0w = s.kv0w;
  *qt0 = s.qt0;
  return 0;
}

// A block of S_q query rows against S_kv key rows, each a multiple of 256;
// a square block is S_q == S_kv. Only non-causal blocks may be rectangular.
static inline bool attn_rect_shape_ok(int batch, int n_heads, int n_kv_heads,
                                      int S_q, int S_kv, bool causal) {
  return attn_block_shape_ok(batch, n_heads, n_kv_heads, S_q) &&
         attn_block_shape_ok(batch, n_heads, n_kv_heads, S_kv) &&
         !(causal && S_q != S_kv);
}

// Bytes of fp32 workspace the backward of an S_q x S_kv block needs right
// now; 0 = the unsplit path. The partials are kv rows, dk [B,H,S_kv,128]
// then dv, and the split rule counts kv workgroups. Host only.
extern "C" long attn_bwd_ws_bytes_rect(int batch, int n_heads, int n_kv_heads,
                                       int S_q, int S_kv, int causal) {
  if (!attn_rect_shape_ok(batch, n_heads, n_kv_heads, S_q, S_kv, causal != 0))
    return 0;
  if (!attn_bwd_use_split(batch, n_heads, n_kv_heads, S_kv, causal != 0))
    return 0;
  return 2L * batch * n_heads * S_kv * ATTN_D * (long)sizeof(float);
}

// the square case
extern "C" long attn_bwd_ws_bytes(int batch, int n_heads, int n_kv_heads,
                                  int S, int causal) {
  return attn_bwd_ws_bytes_rect(batch, n_heads, n_kv_heads, S, S, causal);
}

// dq + dv + dk from given lse and delta (dense [B,H,S] fp32). ws != null
// selects the split dv/dk (the caller has checked its size). S is the q
// length and sizes the dq grid; S_kv (== S when CAUSAL) sizes the dv/dk
// grids, the workspace halves and the reduction.
template <bool CAUSAL>
static void launch_bwd_core(hipStream_t st, const void* q, const void* k,
                            const void* v, const void* dout,
                            const void* lse, const void* delta,
                            void* dq, void* dk, void* dv,
                            AttnStride qs, AttnStride ks, AttnStride vs,
                            AttnStride dos, AttnStride dqs, AttnStride dks,
                            AttnStride dvs, int batch, int n_heads,
                            int n_kv_heads, int S, int S_kv, float scale,
                            void* ws) {
  constexpr int MASK = CAUSAL ? ATTN_MASK_CAUSAL : ATTN_MASK_NONE;
  const int* const no_bounds = nullptr;
  const int sched = attn_sched_mode();
  {
    dim3 grid((S / 256) * n_heads * batch), block(512);
    hipLaunchKernelGGL(attn_bwd_dq_kernel<MASK>, grid, block, 0, st,
                       (const u16*)q, (const u16*)k, (const u16*)v,
                       (const u16*)dout, (const float*)lse,
                       (const float*)delta, (u16*)dq,
                       ATTN_S3(qs), ATTN_S3(ks),
                       ATTN_S3(vs), ATTN_S3(dos),
                       ATTN_S3(dqs),
                       n_heads, n_heads / n_kv_heads, S, scale, batch, sched,
                       S_kv, no_bounds);
  }
  const int nrb = S_kv / 256;
  const bool split = ws != nullptr;
  float* ws_k = (float*)ws;
  float* ws_v = split ? ws_k + (long)batch * n_heads * S_kv * ATTN_D : nullptr;
  const int fold_v = attn_bwd_use_fold(batch, n_heads, n_kv_heads, S_kv,
                                       CAUSAL, split, ATTN_BWD_DV);
  const int fold_k = attn_bwd_use_fold(batch, n_heads, n_kv_heads, S_kv,
                                       CAUSAL, split, ATTN_BWD_DK);
  dim3 grid(nrb * (split ? n_heads : n_kv_heads) * batch), block(512);
  if (fold_v == ATTN_STRIPS_PAIR) {          // causal and unsplit only
    hipLaunchKernelGGL(attn_bwd_dv_pair_kernel, grid, block, 0, st,
                       (const u16*)q, (const u16*)k, (const u16*)dout,
                       (const float*)lse, (u16*)dv,
                       ATTN_S3(qs), ATTN_S3(ks),
                       ATTN_S3(dos), ATTN_S3(dvs),
                       n_heads, n_kv_heads, S, scale, batch, sched);
  } else {
    auto dv_kernel = split ? attn_bwd_dv_kernel<MASK, true>
                           : attn_bwd_dv_kernel<MASK, false>;
    hipLaunchKernelGGL(dv_kernel, grid, block, 0, st,
                       (const u16*)q, (const u16*)k, (const u16*)dout,
                       (const float*)lse, (u16*)dv,
                       ATTN_S3(qs), ATTN_S3(ks),
                       ATTN_S3(dos), ATTN_S3(dvs),
                       n_heads, n_kv_heads, S, scale, ws_v, batch, sched,
                       fold_v, S_kv, no_bounds);
  }
  if (fold_k == ATTN_STRIPS_PAIR) {
    hipLaunchKernelGGL(attn_bwd_dk_pair_kernel, grid, block, 0, st,
                       (const u16*)q, (const u16*)k, (const u16*)v,
                       (const u16*)dout, (const float*)lse,
                       (const float*)delta, (u16*)dk,
                       ATTN_S3(qs), ATTN_S3(ks),
                       ATTN_S3(vs), ATTN_S3(dos),
                       ATTN_S3(dks),
                       n_heads, n_kv_heads, S, scale, batch, sched);
  } else {
    auto dk_kernel = split ? attn_bwd_dk_kernel<MASK, true>
                           : attn_bwd_dk_kernel<MASK, false>;
    hipLaunchKernelGGL(dk_kernel, grid, block, 0, st,
                       (const u16*)q, (const u16*)k, (const u16*)v,
                       (const u16*)dout, (const float*)lse,
                       (const float*)delta, (u16*)dk,
                       ATTN_S3(qs), ATTN_S3(ks),
                       ATTN_S3(vs), ATTN_S3(dos),
                       ATTN_S3(dks),
                       n_heads, n_kv_heads, S, scale, ws_k, batch, sched,
                       fold_k, S_kv, no_bounds);
  }
  if (split) {
    const long n_rows = (long)batch * n_kv_heads * S_kv;
    hipLaunchKernelGGL(attn_bwd_reduce_kernel,
                       dim3((unsigned)((n_rows + 15) / 16), 2), dim3(256), 0,
                       st, (const float*)ws_k, (const float*)ws_v,
                       (u16*)dk, (u16*)dv, ATTN_S3(dks),
                       ATTN_S3(dvs), n_heads, n_kv_heads, S_kv,
                       n_rows);
  }
}

// everything one backward call needs besides its stream and workspace
struct AttnBwdArgs {
  const void *q, *k, *v, *out, *dout, *lse;
  void *delta, *dq, *dk, *dv;
  AttnStride qs, ks, vs, os, dos, dqs, dks, dvs;
  int batch, n_heads, n_kv_heads, S;
  float scale;
  bool causal;
  bool with_delta;     // compute delta from out/dout first (dense entries)
  int S_kv = 0;        // k/v rows of a rectangular block; 0 = square (S)
};

// Shape check of one backward call and the workspace bytes it needs now:
// -1 for a shape the kernels do not cover (rectangular needs non-causal).
static long attn_bwd_need(const AttnBwdArgs& a) {
  const int S_kv = a.S_kv ? a.S_kv : a.S;
  if (!attn_rect_shape_ok(a.batch, a.n_heads, a.n_kv_heads, a.S, S_kv,
                          a.causal))
    return -1;
  return attn_bwd_ws_bytes_rect(a.batch, a.n_heads, a.n_kv_heads, a.S, S_kv,
                                a.causal);
}

// Launch with the caller's workspace. Nothing is launched unless the
// workspace covers the path chosen for this call.
static int launch_bwd_ws(hipStream_t st, const AttnBwdArgs& a, void* ws,
                         long ws_bytes) {
  const long need = attn_bwd_need(a);
  if (need < 0) return -1;
  if (need > 0 && (ws == nullptr || ws_bytes < need)) return -2;
  if (need == 0) ws = nullptr;
  const int S_kv = a.S_kv ? a.S_kv : a.S;
  if (a.with_delta)
    launch_delta(st, a.out, a.dout, a.delta, a.os, a.dos, a.batch, a.n_heads,
                 a.S);
  if (a.causal)
    launch_bwd_core<true>(st, a.q, a.k, a.v, a.dout, a.lse, a.delta, a.dq,
                          a.dk, a.dv, a.qs, a.ks, a.vs, a.dos, a.dqs, a.dks,
                          a.dvs, a.batch, a.n_heads, a.n_kv_heads, a.S, S_kv,
                          a.scale, ws);
  else
    launch_bwd_core<false>(st, a.q, a.k, a.v, a.dout, a.lse, a.delta, a.dq,
                           a.dk, a.dv, a.qs, a.ks, a.vs, a.dos, a.dqs, a.dks,
                           a.dvs, a.batch, a.n_heads, a.n_kv_heads, a.S, S_kv,
                           a.scale, ws);
  return 0;
}

// The entries without a workspace argument make the same choice and, for
// the split path, take a transient workspace ordered on the call's stream
// (stream-ordered allocate, launch, stream-ordered free). That cannot be
// recorded into a graph, so they refuse a capturing stream: callers that
// capture use the _ws entries with memory from their own allocator.
static int launch_bwd_transient(hipStream_t st, const AttnBwdArgs& a) {
  const long need = attn_bwd_need(a);
  if (need < 0) return -1;
  if (need == 0) return launch_bwd_ws(st, a, nullptr, 0);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess ||
      cs != hipStreamCaptureStatusNone)
    return -3;
  void* ws = nullptr;
  if (hipMallocAsync(&ws, (size_t)need, st) != hipSuccess || !ws) return -4;
  const int rc = launch_bwd_ws(st, a, ws, need);
  if (hipFreeAsync(ws, st) != hipSuccess) return -5;
  return rc;
}

// Every backward entry comes as a pair: X takes a transient workspace, X_ws
// the caller's (attn_bwd_ws_bytes[_rect]; may be null when that is 0).
struct AttnWs { bool given; void* ptr; long bytes; };
static const AttnWs ATTN_WS_TRANSIENT = {false, nullptr, 0};

static int launch_bwd(void* stream, const AttnBwdArgs& a, AttnWs ws) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return ws.given ? launch_bwd_ws(st, a, ws.ptr, ws.bytes)
                  : launch_bwd_transient(st, a);
}

// out, dout, dq: dense [B,H,S,D]; dk, dv: dense [B,HKV,S,D]
static int attn_bwd_dense(void* stream, const void* q, const void* k,
                          const void* v, const void* out, const void* dout,
                          const void* lse, void* delta, void* dq, void* dk,
                          void* dv, AttnStride qs, AttnStride ks,
                          AttnStride vs, int batch, int n_heads,
                          int n_kv_heads, int S, float scale, AttnWs ws) {
  const AttnStride dh = attn_dense_stride(n_heads, S);
  const AttnStride dkv = attn_dense_stride(n_kv_heads, S);
  return launch_bwd(stream,
                    AttnBwdArgs{q, k, v, out, dout, lse, delta, dq, dk, dv,
                                qs, ks, vs, dh, dh, dh, dkv, dkv, batch,
                                n_heads, n_kv_heads, S, scale, true, true},
                    ws);
}

extern "C" int attn_bwd(void* stream, const void* q, const void* k,
                        const void* v, const void* out, const void* dout,
                        const void* lse, void* delta,
                        void* dq, void* dk, void* dv,
                        long q_sb, long q_sh, long q_ss,
                        long k_sb, long k_sh, long k_ss,
                        long v_sb, long v_sh, long v_ss,
                        int batch, int n_heads, int n_kv_heads, int S,
                        float scale) {
  return attn_bwd_dense(stream, q, k, v, out, dout, lse, delta, dq, dk, dv,
                        {q_sb, q_sh, q_ss}, {k_sb, k_sh, k_ss},
                        {v_sb, v_sh, v_ss}, batch, n_heads, n_kv_heads, S,
                        scale, ATTN_WS_TRANSIENT);
}

extern "C" int attn_bwd_ws(void* stream, const void* q, const void* k,
                           const void* v, const void* out, const void* dout,
                           const void* lse, void* delta,
                           void* dq, void* dk, void* dv,
                           long q_sb, long q_sh, long q_ss,
                           long k_sb, long k_sh, long k_ss,
                           long v_sb, long v_sh, long v_ss,
                           int batch, int n_heads, int n_kv_heads, int S,
                           float scale, void* ws, long ws_bytes) {
  return attn_bwd_dense(stream, q, k, v, out, dout, lse, delta, dq, dk, dv,
                        {q_sb, q_sh, q_ss}, {k_sb, k_sh, k_ss},
                        {v_sb, v_sh, v_ss}, batch, n_heads, n_kv_heads, S,
                        scale, {true, ws, ws_bytes});
}

// attn_bwd with batch/head/row strides for every [.,.,S,128] operand, so
// the gradients can land in head ranges of one packed [B,S,(H+2HKV)*128]
// buffer and dout can arrive as [B,S,H*128]. st: 8 stride triples in the
// order q, k, v, out, dout, dq, dk, dv.
static int attn_bwd_strided_any(
    void* stream, const void* q, const void* k, const void* v,
    const void* out, const void* dout, const void* lse, void* delta,
    void* dq, void* dk, void* dv, const long* st, int batch, int n_heads,
    int n_kv_heads, int S, float scale, AttnWs ws) {
  if (!st || !attn_strides_ok(st, 24)) return -1;
  return launch_bwd(
      stream,
      AttnBwdArgs{q, k, v, out, dout, lse, delta, dq, dk, dv,
                  attn_stride_at(st, 0), attn_stride_at(st, 1),
                  attn_stride_at(st, 2), attn_stride_at(st, 3),
                  attn_stride_at(st, 4), attn_stride_at(st, 5),
                  attn_stride_at(st, 6), attn_stride_at(st, 7), batch,
                  n_heads, n_kv_heads, S, scale, true, true},
      ws);
}

extern "C" int attn_bwd_strided(void* stream, const void* q, const void* k,
                                const void* v, const void* out,
                                const void* dout, const void* lse,
                                void* delta, void* dq, void* dk, void* dv,
                                const long* st, int batch, int n_heads,
                                int n_kv_heads, int S, float scale) {
  return attn_bwd_strided_any(stream, q, k, v, out, dout, lse, delta, dq, dk,
                              dv, st, batch, n_heads, n_kv_heads, S, scale,
                              ATTN_WS_TRANSIENT);
}

extern "C" int attn_bwd_strided_ws(void* stream, const void* q, const void* k,
                                   const void* v, const void* out,
                                   const void* dout, const void* lse,
                                   void* delta, void* dq, void* dk, void* dv,
                                   const long* st, int batch, int n_heads,
                                   int n_kv_heads, int S, float scale,
                                   void* ws, long ws_bytes) {
  return attn_bwd_strided_any(stream, q, k, v, out, dout, lse, delta, dq, dk,
                              dv, st, batch, n_heads, n_kv_heads, S, scale,
                              {true, ws, ws_bytes});
}

extern "C" int attn_fwd_v7(void* stream, const void* q, const void* k,
                           const void* v, void* out, void* lse,
                           long q_sb, long q_sh, long q_ss,
                           long k_sb, long k_sh, long k_ss,
                           long v_sb, long v_sh, long v_ss,
                           int batch, int n_heads, int n_kv_heads, int S,
                           float scale) {
  if (S <= 0 || S % 256 != 0 || n_heads % n_kv_heads != 0) return -1;
  return launch_fwd_v7(stream, q, k, v, out, lse, {q_sb, q_sh, q_ss},
                       {k_sb, k_sh, k_ss}, {v_sb, v_sh, v_ss},
                       attn_dense_stride(n_heads, S), batch, n_heads,
                       n_kv_heads, S, scale);
}

// v7 forward with `out` through batch/head/row strides as well (lse stays
// dense [B,H,S]); S % 256 == 0 only. st: 4 stride triples q, k, v, out.
extern "C" int attn_fwd_strided(void* stream, const void* q, const void* k,
                                const void* v, void* out, void* lse,
                                const long* st, int batch, int n_heads,
                                int n_kv_heads, int S, float scale) {
  if (S <= 0 || S % 256 != 0 || n_heads <= 0 || batch <= 0 ||
      n_kv_heads <= 0 || n_heads % n_kv_heads != 0)
    return -1;
  if (!st || !attn_strides_ok(st, 12)) return -1;
  return launch_fwd_v7(stream, q, k, v, out, lse, attn_stride_at(st, 0),
                       attn_stride_at(st, 1), attn_stride_at(st, 2),
                       attn_stride_at(st, 3), batch, n_heads, n_kv_heads, S,
                       scale);
}

// ===========================================================================
// Block entries for ring (context-parallel) attention: one S x S block of a
// longer sequence per call, S_q == S_kv == S. causal != 0 is the diagonal
// block (the kernels above, unchanged); causal == 0 runs the same kernels
// with the tile bound and the mask compiled out, for blocks that lie wholly
// below the diagonal. The backward takes lse and delta as INPUTS so the
// ring can pass the merged (global) statistics: P = 2^(s*scale2 - lse2)
// then is this block's share of the global softmax, and since the global
// lse is >= the block's own, P <= 1 with no clamping.
// Stride triples (batch, head, row) arrive as a host long[] like the
// *_strided entries; lse and delta stay dense [B,H,S] fp32.
// ===========================================================================

// st: 4 triples q, k, v, out
extern "C" int attn_block_fwd(void* stream, const void* q, const void* k,
                              const void* v, void* out, void* lse,
                              const long* st, int batch, int n_heads,
                              int n_kv_heads, int S, float scale,
                              int causal) {
  if (!attn_block_shape_ok(batch, n_heads, n_kv_heads, S)) return -1;
  if (!st || !attn_strides_ok(st, 12)) return -1;
  return launch_fwd_v7(stream, q, k, v, out, lse, attn_stride_at(st, 0),
                       attn_stride_at(st, 1), attn_stride_at(st, 2),
                       attn_stride_at(st, 3), batch, n_heads, n_kv_heads, S,
                       scale, causal != 0);
}

// st: 2 triples out, dout
extern "C" int attn_delta(void* stream, const void* out, const void* dout,
                          void* delta, const long* st, int batch,
                          int n_heads, int S) {
  if (S <= 0 || S % 16 != 0 || n_heads <= 0 || batch <= 0) return -1;
  if (!st || !attn_strides_ok(st, 6)) return -1;
  launch_delta(reinterpret_cast<hipStream_t>(stream), out, dout, delta,
               attn_stride_at(st, 0), attn_stride_at(st, 1), batch, n_heads,
               S);
  return 0;
}

// st: 7 triples q, k, v, dout, dq, dk, dv. S_kv: k/v rows of a rectangular
// block, 0 = square.
static int attn_block_bwd_any(
    void* stream, const void* q, const void* k, const void* v,
    const void* dout, const void* lse, const void* delta, void* dq, void* dk,
    void* dv, const long* st, int batch, int n_heads, int n_kv_heads, int S,
    int S_kv, float scale, int causal, AttnWs ws) {
  if (!st || !attn_strides_ok(st, 21)) return -1;
  // delta is an input here: never written, no out operand
  return launch_bwd(
      stream,
      AttnBwdArgs{q, k, v, nullptr, dout, lse, const_cast<void*>(delta), dq,
                  dk, dv, attn_stride_at(st, 0), attn_stride_at(st, 1),
                  attn_stride_at(st, 2), AttnStride{0, 0, 0},
                  attn_stride_at(st, 3), attn_stride_at(st, 4),
                  attn_stride_at(st, 5), attn_stride_at(st, 6), batch,
                  n_heads, n_kv_heads, S, scale, causal != 0, false, S_kv},
      ws);
}

extern "C" int attn_block_bwd(void* stream, const void* q, const void* k,
                              const void* v, const void* dout,
                              const void* lse, const void* delta,
                              void* dq, void* dk, void* dv,
                              const long* st, int batch, int n_heads,
                              int n_kv_heads, int S, float scale,
                              int causal) {
  return attn_block_bwd_any(stream, q, k, v, dout, lse, delta, dq, dk, dv, st,
                            batch, n_heads, n_kv_heads, S, 0, scale, causal,
                            ATTN_WS_TRANSIENT);
}

extern "C" int attn_block_bwd_ws(void* stream, const void* q, const void* k,
                                 const void* v, const void* dout,
                                 const void* lse, const void* delta,
                                 void* dq, void* dk, void* dv,
                                 const long* st, int batch, int n_heads,
                                 int n_kv_heads, int S, float scale,
                                 int causal, void* ws, long ws_bytes) {
  return attn_block_bwd_any(stream, q, k, v, dout, lse, delta, dq, dk, dv, st,
                            batch, n_heads, n_kv_heads, S, 0, scale, causal,
                            {true, ws, ws_bytes});
}

// Rectangular blocks: S_q query rows against S_kv key rows (each a multiple
// of 256), non-causal unless S_q == S_kv. The zig-zag ring visits the low
// half of a K/V shard with all q rows and a whole K/V shard with the high
// half of the q rows. lse and delta are dense fp32 [B,H,S_q]; dk and dv have
// S_kv rows. A square shape computes what the square entries compute.
extern "C" int attn_block_fwd_rect(void* stream, const void* q, const void* k,
                                   const void* v, void* out, void* lse,
                                   const long* st, int batch, int n_heads,
                                   int n_kv_heads, int S_q, int S_kv,
                                   float scale, int causal) {
  if (!attn_rect_shape_ok(batch, n_heads, n_kv_heads, S_q, S_kv, causal != 0))
    return -1;
  if (!st || !attn_strides_ok(st, 12)) return -1;
  return launch_fwd_v7(stream, q, k, v, out, lse, attn_stride_at(st, 0),
                       attn_stride_at(st, 1), attn_stride_at(st, 2),
                       attn_stride_at(st, 3), batch, n_heads, n_kv_heads, S_q,
                       scale, causal != 0, S_kv);
}

static int attn_block_bwd_rect_any(
    void* stream, const void* q, const void* k, const void* v,
    const void* dout, const void* lse, const void* delta, void* dq, void* dk,
    void* dv, const long* st, int batch, int n_heads, int n_kv_heads,
    int S_q, int S_kv, float scale, int causal, AttnWs ws) {
  if (S_kv <= 0) return -1;              // 0 would mean square below
  return attn_block_bwd_any(stream, q, k, v, dout, lse, delta, dq, dk, dv, st,
                            batch, n_heads, n_kv_heads, S_q, S_kv, scale,
                            causal, ws);
}

extern "C" int attn_block_bwd_rect(void* stream, const void* q, const void* k,
                                   const void* v, const void* dout,
                                   const void* lse, const void* delta,
                                   void* dq, void* dk, void* dv,
                                   const long* st, int batch, int n_heads,
                                   int n_kv_heads, int S_q, int S_kv,
                                   float scale, int causal) {
  return attn_block_bwd_rect_any(stream, q, k, v, dout, lse, delta, dq, dk,
                                 dv, st, batch, n_heads, n_kv_heads, S_q,
                                 S_kv, scale, causal, ATTN_WS_TRANSIENT);
}

extern "C" int attn_block_bwd_rect_ws(void* stream, const void* q,
                                      const void* k, const void* v,
                                      const void* dout, const void* lse,
                                      const void* delta, void* dq, void* dk,
                                      void* dv, const long* st, int batch,
                                      int n_heads, int n_kv_heads, int S_q,
                                      int S_kv, float scale, int causal,
                                      void* ws, long ws_bytes) {
  return attn_block_bwd_rect_any(stream, q, k, v, dout, lse, delta, dq, dk,
                                 dv, st, batch, n_heads, n_kv_heads, S_q,
                                 S_kv, scale, causal, {true, ws, ws_bytes});
}

// o_acc fp32 dense [B,H,S,128]; lse_acc, lse_blk fp32 dense [B,H,S];
// o_blk bf16 through st: 1 triple (batch, head, row)
extern "C" int attn_merge(void* stream, void* o_acc, void* lse_acc,
                          const void* o_blk, const void* lse_blk,
                          const long* st, int batch, int n_heads, int S) {
  if (S <= 0 || n_heads <= 0 || batch <= 0) return -1;
  if (!st || !attn_strides_ok(st, 3)) return -1;
  const long n_rows = (long)batch * n_heads * S;
  const long n_blocks = (n_rows + 15) / 16;
  if (n_blocks > 0x7fffffffL) return -1;
  hipLaunchKernelGGL(attn_merge_kernel, dim3((unsigned)n_blocks), dim3(256),
                     0, reinterpret_cast<hipStream_t>(stream),
                     (float*)o_acc, (float*)lse_acc, (const u16*)o_blk,
                     (const float*)lse_blk, st[0], st[1], st[2],
                     n_heads, S, n_rows);
  return 0;
}

// ===========================================================================
// Document-masked entries (see the kernels). bounds: int32 [2, B, S] on the
// device, start rows then end rows. Both entries launch nothing and return
// nonzero on S % 256 != 0, n_heads % n_kv_heads != 0, a null bounds or bad
// strides. dv and dk always run the identity ownership, unsplit:
// AITJ_ATTN_BWD_FOLD and AITJ_ATTN_BWD_SPLIT do not apply, and there is no
// workspace. AITJ_ATTN_SCHED applies as everywhere.
// ===========================================================================

// Host-callable twin of the clamped tile ranges (tests/
// test_doc_attention_cpu.py). kind 0: the kv tiles [first, last] that q block
// `block` walks in the forward and dq when bounds[0] of its first row is
// start_or_end; kind 1: the q tiles kv block `block` walks in dv and dk when
// bounds[1] of its last row is start_or_end. Any int value is accepted, as
// in the kernels. Returns nonzero for arguments outside a launch.
extern "C" int attn_doc_tiles_decode(int kind, int start_or_end, int block,
                                     int S, int* first, int* last) {
  if (S <= 0 || S % 256 != 0 || block < 0 || block >= S / 256 ||
      (kind != 0 && kind != 1))
    return -1;
  const AttnTiles t = kind == 0 ? attn_doc_tiles_q(start_or_end, block)
                                : attn_doc_tiles_kv(start_or_end, block, S);
  *first = t.first;
  *last = t.last;
  return 0;
}

// st: 4 stride triples q, k, v, out (lse dense [B,H,S])
extern "C" int attn_doc_fwd_strided(void* stream, const void* q,
                                    const void* k, const void* v, void* out,
                                    void* lse, const int* bounds,
                                    const long* st, int batch, int n_heads,
                                    int n_kv_heads, int S, float scale) {
  if (!attn_block_shape_ok(batch, n_heads, n_kv_heads, S) || !bounds)
    return -1;
  if (!st || !attn_strides_ok(st, 12)) return -1;
  const AttnStride qs = attn_stride_at(st, 0), ks = attn_stride_at(st, 1),
                   vs = attn_stride_at(st, 2), os = attn_stride_at(st, 3);
  dim3 grid((S / 256) * n_heads * batch), block(512);
  hipLaunchKernelGGL(attn_fwd_v7_kernel<ATTN_MASK_DOC>, grid, block, 0,
                     reinterpret_cast<hipStream_t>(stream),
                     (const u16*)q, (const u16*)k, (const u16*)v, (u16*)out,
                     (float*)lse, ATTN_S3(qs), ATTN_S3(ks),
                     ATTN_S3(vs), ATTN_S3(os), n_heads, n_heads / n_kv_heads,
                     S, scale * ATTN_LOG2E, batch, attn_sched_mode(), S,
                     bounds);
  return 0;
}

// delta (with_delta) and the kernels named by parts. Every training entry
// passes ATTN_PART_ALL; attn_bwd_part, the timing entry, names one.
#define ATTN_PART_DQ 1
#define ATTN_PART_DV 2
#define ATTN_PART_DK 4
#define ATTN_PART_ALL 7
static int launch_doc_bwd(void* stream, const void* q, const void* k,
                          const void* v, const void* out, const void* dout,
                          const void* lse, void* delta, void* dq, void* dk,
                          void* dv, const int* bounds, const long* st,
                          int batch, int n_heads, int n_kv_heads, int S,
                          float scale, bool with_delta, int parts) {
  if (!attn_block_shape_ok(batch, n_heads, n_kv_heads, S) || !bounds)
    return -1;
  if (!st || !attn_strides_ok(st, 24)) return -1;
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  const AttnStride qs = attn_stride_at(st, 0), ks = attn_stride_at(st, 1),
                   vs = attn_stride_at(st, 2), os = attn_stride_at(st, 3),
                   dos = attn_stride_at(st, 4), dqs = attn_stride_at(st, 5),
                   dks = attn_stride_at(st, 6), dvs = attn_stride_at(st, 7);
  const int sched = attn_sched_mode();
  if (with_delta)
    launch_delta(hs, out, dout, delta, os, dos, batch, n_heads, S);
  if (parts & ATTN_PART_DQ) {
    hipLaunchKernelGGL(attn_bwd_dq_kernel<ATTN_MASK_DOC>,
                       dim3((S / 256) * n_heads * batch), dim3(512), 0, hs,
                       (const u16*)q, (const u16*)k, (const u16*)v,
                       (const u16*)dout, (const float*)lse,
                       (const float*)delta, (u16*)dq, ATTN_S3(qs),
                       ATTN_S3(ks), ATTN_S3(vs), ATTN_S3(dos), ATTN_S3(dqs),
                       n_heads, n_heads / n_kv_heads, S, scale, batch, sched,
                       S, bounds);
  }
  // unsplit, no workspace; the document mode does not read the strip flag
  dim3 grid((S / 256) * n_kv_heads * batch), block(512);
  if (parts & ATTN_PART_DV) {
    hipLaunchKernelGGL((attn_bwd_dv_kernel<ATTN_MASK_DOC, false>), grid,
                       block, 0, hs,
                       (const u16*)q, (const u16*)k, (const u16*)dout,
                       (const float*)lse, (u16*)dv, ATTN_S3(qs),
                       ATTN_S3(ks), ATTN_S3(dos), ATTN_S3(dvs), n_heads,
                       n_kv_heads, S, scale, (float*)nullptr, batch, sched,
                       ATTN_STRIPS_IDENTITY, S, bounds);
  }
  if (parts & ATTN_PART_DK) {
    hipLaunchKernelGGL((attn_bwd_dk_kernel<ATTN_MASK_DOC, false>), grid,
                       block, 0, hs,
                       (const u16*)q, (const u16*)k, (const u16*)v,
                       (const u16*)dout, (const float*)lse,
                       (const float*)delta, (u16*)dk, ATTN_S3(qs),
                       ATTN_S3(ks), ATTN_S3(vs), ATTN_S3(dos), ATTN_S3(dks),
                       n_heads, n_kv_heads, S, scale, (float*)nullptr, batch,
                       sched, ATTN_STRIPS_IDENTITY, S, bounds);
  }
  return 0;
}

// delta, dq, dv, dk. st: 8 stride triples q, k, v, out, dout, dq, dk, dv
// (lse and delta dense [B,H,S]; delta is written first, then read)
extern "C" int attn_doc_bwd_strided(void* stream, const void* q,
                                    const void* k, const void* v,
                                    const void* out, const void* dout,
                                    const void* lse, void* delta, void* dq,
                                    void* dk, void* dv, const int* bounds,
                                    const long* st, int batch, int n_heads,
                                    int n_kv_heads, int S, float scale) {
  return launch_doc_bwd(stream, q, k, v, out, dout, lse, delta, dq, dk, dv,
                        bounds, st, batch, n_heads, n_kv_heads, S, scale,
                        true, ATTN_PART_ALL);
}

// One backward kernel alone, for per-kernel timing (scripts/
// attndocbench.py): part 1 dq, 2 dv, 4 dk. lse and delta are inputs. With
// bounds the document kernel; with null bounds the causal unsplit launch,
// dv/dk under the ownership the causal entries would pick for the shape
// now. st: 8 triples as in attn_bwd_strided (out unused).
extern "C" int attn_bwd_part(void* stream, const void* q, const void* k,
                             const void* v, const void* dout,
                             const void* lse, const void* delta, void* dq,
                             void* dk, void* dv, const int* bounds,
                             const long* st, int batch, int n_heads,
                             int n_kv_heads, int S, float scale, int part) {
  if (part != ATTN_PART_DQ && part != ATTN_PART_DV && part != ATTN_PART_DK)
    return -1;
  if (bounds)
    return launch_doc_bwd(stream, q, k, v, nullptr, dout, lse,
                          const_cast<void*>(delta), dq, dk, dv, bounds, st,
                          batch, n_heads, n_kv_heads, S, scale, false, part);
  if (!attn_block_shape_ok(batch, n_heads, n_kv_heads, S)) return -1;
  if (!st || !attn_strides_ok(st, 24)) return -1;
  // A launcher of its own, so that no benchmark switch sits in
  // launch_bwd_core: the causal unsplit launch of that one kernel, with the
  // ownership launch_bwd_core would pick (attn_bwd_use_fold). bounds is null
  // from here on.
  hipStream_t hs = reinterpret_cast<hipStream_t>(stream);
  const AttnStride qs = attn_stride_at(st, 0), ks = attn_stride_at(st, 1),
                   vs = attn_stride_at(st, 2), dos = attn_stride_at(st, 4),
                   dqs = attn_stride_at(st, 5), dks = attn_stride_at(st, 6),
                   dvs = attn_stride_at(st, 7);
  const int sched = attn_sched_mode();
  dim3 grid((S / 256) * n_kv_heads * batch), block(512);
  if (part == ATTN_PART_DQ) {
    hipLaunchKernelGGL(attn_bwd_dq_kernel<ATTN_MASK_CAUSAL>,
                       dim3((S / 256) * n_heads * batch), block, 0, hs,
                       (const u16*)q, (const u16*)k, (const u16*)v,
                       (const u16*)dout, (const float*)lse,
                       (const float*)delta, (u16*)dq, ATTN_S3(qs),
                       ATTN_S3(ks), ATTN_S3(vs), ATTN_S3(dos), ATTN_S3(dqs),
                       n_heads, n_heads / n_kv_heads, S, scale, batch, sched,
                       S, bounds);
  } else if (part == ATTN_PART_DV) {
    const int fold = attn_bwd_use_fold(batch, n_heads, n_kv_heads, S, true,
                                       false, ATTN_BWD_DV);
    if (fold == ATTN_STRIPS_PAIR)
      hipLaunchKernelGGL(attn_bwd_dv_pair_kernel, grid, block, 0, hs,
                         (const u16*)q, (const u16*)k, (const u16*)dout,
                         (const float*)lse, (u16*)dv, ATTN_S3(qs),
                         ATTN_S3(ks), ATTN_S3(dos), ATTN_S3(dvs), n_heads,
                         n_kv_heads, S, scale, batch, sched);
    else
      hipLaunchKernelGGL((attn_bwd_dv_kernel<ATTN_MASK_CAUSAL, false>), grid,
                         block, 0,
                         hs, (const u16*)q, (const u16*)k, (const u16*)dout,
                         (const float*)lse, (u16*)dv, ATTN_S3(qs),
                         ATTN_S3(ks), ATTN_S3(dos), ATTN_S3(dvs), n_heads,
                         n_kv_heads, S, scale, (float*)nullptr, batch, sched,
                         fold, S, bounds);
  } else {
    const int fold = attn_bwd_use_fold(batch, n_heads, n_kv_heads, S, true,
                                       false, ATTN_BWD_DK);
    if (fold == ATTN_STRIPS_PAIR)
      hipLaunchKernelGGL(attn_bwd_dk_pair_kernel, grid, block, 0, hs,
                         (const u16*)q, (const u16*)k, (const u16*)v,
                         (const u16*)dout, (const float*)lse,
                         (const float*)delta, (u16*)dk, ATTN_S3(qs),
                         ATTN_S3(ks), ATTN_S3(vs), ATTN_S3(dos), ATTN_S3(dks),
                         n_heads, n_kv_heads, S, scale, batch, sched);
    else
      hipLaunchKernelGGL((attn_bwd_dk_kernel<ATTN_MASK_CAUSAL, false>), grid,
                         block, 0,
                         hs, (const u16*)q, (const u16*)k, (const u16*)v,
                         (const u16*)dout, (const float*)lse,
                         (const float*)delta, (u16*)dk, ATTN_S3(qs),
                         ATTN_S3(ks), ATTN_S3(vs), ATTN_S3(dos), ATTN_S3(dks),
                         n_heads, n_kv_heads, S, scale, (float*)nullptr,
                         batch, sched, fold, S, bounds);
  }
  return 0;
}

#undef ATTN_S3
