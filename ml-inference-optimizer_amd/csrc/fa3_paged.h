// Paged form of the pipelined attention kernels (mio_fa3_fwd_paged): chunked prefill, prefix sharing and multi-token verify
// over the paged KV cache, without gathering the context into a contiguous buffer.
//
// q / o [total_q, H, D] packed as in varlen (fa3_varlen.h: cu_seqlens_q, lse fp32 [H, total_q]).  K / V come from the cache
// [num_blocks, L, block_size, Hkv, D] (contiguous) at layer `layer`: sequence b owns key positions 0 .. Lk_b - 1, Lk_b =
// min(seqused_k[b], max_seqlen_k, max_blocks * block_size), and key j lives in page block_tables[b, j / block_size] at slot
// j % block_size.  Causal is bottom-right aligned (q_offset = Lk - Lq).  The grid, the XCD remap, the early exits and the
// empty-sequence writer are the varlen kernels' (fa_seq_prepare); the bodies are the dense ones with FA_KV_TILE below.
//
// block_size % 64 == 0, so a 64-key tile never spans two pages: within the tile the rows are at the cache's token stride
// exactly as in a dense K / V, the per-lane DMA offsets stay as they are, and only the tile's scalar base changes:
//   cache + ((page * L + layer) * block_size + (64 t) % block_size) * Hkv * D  elements,
// as a 32-bit row index (the launcher refuses caches of 2^32 rows or more) times the row size in 64 bits.
//
// Page lookups (FaPageWalk) never stand in front of a tile's DMA: the table entries come through scalar loads in windows of
// two logical blocks, and the window that follows is requested as soon as one is entered -- at block size 64 that is two
// tiles (one or two DMA batches) before it is needed.  When a window runs past the pass' last tile, the window requested is
// block 0: the first tiles of the next pass (fwd5 primes them from the heavy pass' last iterations, fwd3 from its pass start)
// and fwd3's re-fetch of the last tile past the end both hit a window that is already there.  A lookup outside both windows
// (never on these walks) loads its window synchronously.  Every table read has its logical block clamped into
// [0, max_blocks) and every page into [0, num_blocks): a bad table gives wrong numbers, never an out-of-bounds access.
#pragma once
#include "fa3_fwd3_kernel.h"
#include "fa3_fwd5_kernel.h"
#include "fa3_varlen.h"

struct FaPaged {
  const int32_t* cu_q;          // [B + 1] device
  const int32_t* seqused_k;     // [B] device
  const int32_t* block_tables;  // [B, max_blocks] device
  int total_q, max_q;
  int max_k;                    // min(max_seqlen_k, max_blocks * block_size)
  int num_blocks, num_layers, layer, block_size, max_blocks;
  int tpb;                      // tiles per page: block_size / 64
  uint32_t tpb_magic;           // ceil(2^31 / tpb): lb = mulhi(2 t, tpb_magic) = t / tpb for every tile index t here
};

// Batch entry b's sequence: queries as in fa_varlen_seq, keys 0 .. Lk - 1 of its pages (k0 = 0)
__device__ __forceinline__ FaSeq fa_seq_of(const FaPaged& g, int b) {
  auto clamp = [](int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); };
  FaSeq s;
  s.q0 = clamp(__builtin_amdgcn_readfirstlane(g.cu_q[b]), 0, g.total_q);
  const int q1 = clamp(__builtin_amdgcn_readfirstlane(g.cu_q[b + 1]), s.q0, g.total_q);
  s.Lq = q1 - s.q0 < g.max_q ? q1 - s.q0 : g.max_q;
  s.k0 = 0;
  s.Lk = clamp(__builtin_amdgcn_readfirstlane(g.seqused_k[b]), 0, g.max_k);
  return s;
}

using fa_cint32 = const __attribute__((address_space(4))) int32_t;  // constant address space: scalar (SMEM) loads

// The block-table walk of one workgroup (one sequence); lives in scalar registers.
struct FaPageWalk {
  fa_cint32* row;    // the sequence's block-table row
  int w0, n0;        // first logical block of the current / the requested window
  int wp0, wp1;      // pages of w0, w0 + 1
  int np0, np1;      // pages of n0, n0 + 1 (may still be in flight)

  __device__ __forceinline__ int entry(const FaPaged& g, int lb) const {
    return row[lb < g.max_blocks - 1 ? lb : g.max_blocks - 1];
  }
  __device__ __forceinline__ void init(const FaPaged& g, int b) {
    row = (fa_cint32*)(g.block_tables + (int64_t)b * g.max_blocks);
    w0 = 0;
    wp0 = entry(g, 0);
    wp1 = entry(g, 1);
    n0 = 2;
    np0 = entry(g, 2);
    np1 = entry(g, 3);
  }
  // The scalar K / V bases of tile `tile` of a pass that ends before tile t_end; kbase / vbase: the cache plus this head's
  // offset.  wrap_lb: the logical block requested when a window runs past the pass' end (the next pass' first block).
  __device__ __forceinline__ void tile_base(const FaPaged& g, int tile, int t_end, int wrap_lb, const void* kbase,
                                            const void* vbase, int ks2, int vs2, const char*& kb, const char*& vb) {
    int lb = (int)__umulhi(2u * (uint32_t)tile, g.tpb_magic);
    lb = lb < g.max_blocks - 1 ? lb : g.max_blocks - 1;
    int slot = tile - lb * g.tpb;
    slot = slot < g.tpb - 1 ? slot : g.tpb - 1;
    if ((uint32_t)(lb - w0) >= 2u) {
      if ((uint32_t)(lb - n0) < 2u) {
        w0 = n0;
        wp0 = np0;
        wp1 = np1;
      } else {  // off the walk: load the window now
        w0 = lb;
        wp0 = entry(g, lb);
        wp1 = entry(g, lb + 1);
      }
      n0 = (w0 + 2) * g.tpb < t_end ? w0 + 2 : wrap_lb;  // the rest of this pass, or the next pass' first tiles
      np0 = entry(g, n0);
      np1 = entry(g, n0 + 1);
    }
    int page = lb == w0 ? wp0 : wp1;
    page = page < 0 ? 0 : (page < g.num_blocks - 1 ? page : g.num_blocks - 1);
    const uint32_t r = ((uint32_t)page * (uint32_t)g.num_layers + (uint32_t)g.layer) * (uint32_t)g.block_size +
                       (uint32_t)slot * FA_BN;
    kb = (const char*)kbase + (uint64_t)r * (uint32_t)ks2;
    vb = (const char*)vbase + (uint64_t)r * (uint32_t)vs2;
  }
};

// The walk of a windowed pass (fa3_win_inst.hip, fa3_kv8_inst.hip): tiles are absolute, a pass covers tiles t_lo ..
// t_end - 1, and the window requested when one runs past the pass' end is the first block of the NEXT pass' range
// (t_next), not block 0: tile_base gets (t_end, next_lb).  The first pass starts the walk at its own first block.
struct FaPageWalkWin : FaPageWalk {
  int t_end, next_lb;
  __device__ __forceinline__ void begin_pass(const FaPaged& g, int t_lo, int t_end_, int t_next, bool first) {
    t_end = t_end_;
    next_lb = (int)__umulhi(2u * (uint32_t)t_next, g.tpb_magic);
    if (first) {
      w0 = (int)__umulhi(2u * (uint32_t)t_lo, g.tpb_magic);
      wp0 = entry(g, w0);
      wp1 = entry(g, w0 + 1);
      n0 = (w0 + 2) * g.tpb < t_end ? w0 + 2 : next_lb;
      np0 = entry(g, n0);
      np1 = entry(g, n0 + 1);
    }
  }
};

// Turns the launch's FaDev into this workgroup's dense problem over its sequence's pages and starts the walk (see
// fa_seq_prepare for the exits).  p.k / p.v stay at the cache base: the tile bases come from the walk.
template <int BM, int NT, bool CAUSAL>
__device__ __forceinline__ bool fa_paged_prepare(FaDev& p, const FaPaged& g, FaPageWalk& w) {
  int b;
  if (!fa_seq_prepare<BM, NT, CAUSAL>(p, g, b)) return false;
  w.init(g, b);
  return true;
}

// The layer's scales of an fp8 (e4m3fn) cache, read from device memory: k_scale joins the score scale, v_scale is returned
// for the epilogue's 1 / l (fa3_kv8_inst.hip).
__device__ __forceinline__ float fa_kv8_scales(FaDev& p, const float* k_scale, const float* v_scale) {
  p.scale_log2e *= *k_scale;
  return *v_scale;
}

// FA_KV_TILE of the paged kernels: `walk`, `pg` (FaPaged) come from the kernel, n_tiles / kbase / vbase / ks2 / vs2 from
// the body.  Windowed paged kernels: their FA_KV_TILE, and FA_WIN_PASS of a pass.
#define FA_KV_TILE_PAGED(tile, kb, vb) walk.tile_base(pg, (tile), n_tiles, 0, kbase, vbase, ks2, vs2, kb, vb)
#define FA_KV_TILE_PAGED_WIN(tile, kb, vb) \
  walk.tile_base(pg, (tile), walk.t_end, walk.next_lb, kbase, vbase, ks2, vs2, kb, vb)
#define FA_WIN_PASS_PAGED(t_lo, t_end, t_next, first) walk.begin_pass(pg, (t_lo), (t_end), (t_next), (first))

// padded head dim 64: the fwd5 body (plain K and output) on this workgroup's sequence, K / V tiles through its pages
template <typename T, bool CAUSAL>
__global__ __launch_bounds__(512) void fa3_fwd5_paged_kernel(const FaDev pl, const FaPaged pg) {
  constexpr bool STAMP = false, CARRY = false, OBLK = false, KPRE = false;
  constexpr int ABL = 0;
  FaDev p = pl;
  FaPageWalk walk;
  if (!fa_paged_prepare<FA5_BM, 512, CAUSAL>(p, pg, walk)) return;
#define FA_KV_TILE FA_KV_TILE_PAGED
#define FA_LSE_INDEX(b, head, row) ((int64_t)(head) * pg.total_q + (row))
#include "fa3_fwd5_body.inc"
#undef FA_LSE_INDEX
#undef FA_KV_TILE
}

// padded head dims 96 / 128: the fwd3 body, likewise
template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(256) void fa3_fwd3_paged_kernel(const FaDev pl, const FaPaged pg) {
  constexpr bool STAMP = false, KPRE = false;
  constexpr int ABL = 0;
  FaDev p = pl;
  FaPageWalk walk;
  if (!fa_paged_prepare<FA3_BM, 256, CAUSAL>(p, pg, walk)) return;
#define FA_KV_TILE FA_KV_TILE_PAGED
#define FA_LSE_INDEX(b, head, row) ((int64_t)(head) * pg.total_q + (row))
#include "fa3_fwd3_body.inc"
#undef FA_LSE_INDEX
#undef FA_KV_TILE
}

// Host launchers of the sliding-window forms (fa3_win_inst.hip) for one (dtype, padded D): the dense launch (p as
// mio_fa3_fwd fills it) and the per-sequence launches (p, seq as for fa3_seq_launch).  left / right: -1 = unbounded.
template <typename T, int D>
int fa3_win_launch(const FaDev& p, int causal, int left, int right, hipStream_t stream);
template <typename T, int D, typename V>
int fa3_win_seq_launch(const FaDev& p, const V& seq, int causal, int left, int right, hipStream_t stream);
// Host launcher of the fp8 (e4m3fn) KV-cache forms (fa3_kv8_inst.hip) for one (dtype of q / o, padded D): p and pg as for
// the paged launch, with the cache strides in 16-bit units of the one-byte rows; k_scale / v_scale: device pointers to the
// layer's fp32 scales; left / right: the window, (-1, -1) = none.
template <typename T, int D>
int fa3_kv8_launch(const FaDev& p, const FaPaged& pg, const float* k_scale, const float* v_scale, int causal, int left,
                   int right, hipStream_t stream);
