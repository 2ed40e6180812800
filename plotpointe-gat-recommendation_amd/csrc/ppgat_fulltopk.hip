// ppgat_fulltopk.hip -- full-catalogue top-K recommendation: for every query user the k best
// items outside the user's train history, in one fused pass.
//
//   s(i) = <U[u], I[i]>;  out[b, 0..k) = the first k of { i not in history(u) } under the total
//   order (s descending, i ascending); fewer than k eligible items: the tail is -1 / -inf
//
// The product is the score-tile engine of ppgat_score_tile.h, the one k_full_rank
// (ppgat_fullrank.hip) uses, with that kernel's geometry: a block owns TM queries (32 per wave),
// keeps their user rows as split bf16 B fragments in registers, walks the item table in ascending
// TN-item tiles, builds the history mask per tile from a sorted cursor, and takes the 32x32x16
// product transposed, so a lane holds 16 scores of ONE user.  Fragments, staging, the six-term
// chain and its k order are the same code, so a (user, item) score here is bitwise the score
// k_full_rank compares.  The tile loop and the selection epilogue are this file's own.
//
// Selection epilogue.  The lane's user has a threshold thr (the k-th best score kept so far, -inf
// until k items are kept; both lanes of a user read it from LDS).  A non-masked score passes when
// acc > thr, strictly: items ascend along the walk, so a later item whose score equals the k-th
// kept score has a larger index than every kept item and loses the tie.  A ballot lets the wave
// skip a subtile where nothing passes -- after the first tiles nearly every subtile (the expected
// number of passes per user is about k ln(n_items / k)).  Passing (score, item) pairs are appended
// to the user's candidate buffer of cap = k + 64 (rounded up to 32) entries in a workspace.  The
// buffer's fill count is a register holding the same number in the user's two lanes; the pass
// predicates are lane masks, so each lane sees its partner's bit in the ballot and the two take
// consecutive slots with no atomic at all, and an accumulator register in which no lane passes
// costs one scalar branch.  Before a
// subtile appends, the wave makes sure each of its users has room for 32 more; a user without room
// is compacted by the whole wave: the entries are staged in LDS, each one's position is the number
// of entries that beat it under the total order, the k best are written back in that order and
// thr becomes the k-th.  A compaction stalls its wave and, through the tile barrier, the block;
// the users of a block fill at the same pace, so once one buffer has run full every wave compacts
// its fuller buffers at the start of the next tile, all waves at the same time.  The result is a
// function of the total order alone, whenever the compactions happen: no float atomics, and two
// calls give the same bits.
//
// A launch too small to fill the chip splits the item range over blockIdx.y; each split leaves a
// sorted partial list, and k_full_topk_merge (one wave per query) merges them under the same
// order, pads and writes out_idx / out_score.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ppgat_internal.h"
#include "ppgat_device.h"
#include "ppgat_score_tile.h"

namespace ppgat {
namespace {

using split::f32x16;
using split::mfma32_x6;
using split::u32x4;

constexpr int kFtMaxK = 128;
constexpr int kFtMaxCap = 192;  // ft_cap(kFtMaxK)
constexpr int kFtPerLane = 3;   // ceil(kFtMaxCap / 64)
constexpr int kFtEarly = 16;    // appended entries from which a user joins a block-wide compaction round

// candidate a = (score bits, item) comes before b under (score descending, item ascending)
__device__ __forceinline__ bool ft_beats(float as, uint32_t ai, float bs, uint32_t bi) {
  return as > bs || (as == bs && ai < bi);
}
__device__ __forceinline__ void ft_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }
// between lanes of one wave: LDS and memory instructions of a wave are issued in order, so this only
// keeps the compiler from moving accesses across it
__device__ __forceinline__ void ft_fence_wave() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// k_full_rank's choice: 8 waves (C = 256: 4, one wave per SIMD); 128, 128, 64, 32 items per tile
template <int C>
using FtGeo = score::Geo<C, (C == 256 ? 4 : 8), (C >= 64 ? 8192 / C : 128)>;
template <int C>
struct FtCfg : FtGeo<C> {
  using G = FtGeo<C>;
  static constexpr size_t OFF_MASK = 2 * (size_t)G::BUF;                       // [2][TM][SUB] u32
  static constexpr size_t OFF_CNT = OFF_MASK + 2 * (size_t)G::TM * G::SUB * 4;  // [TM] i32
  static constexpr size_t OFF_THR = OFF_CNT + (size_t)G::TM * 4;                // [TM] f32
  static constexpr size_t OFF_NS = OFF_THR + (size_t)G::TM * 4;                 // [TM] i32
  static constexpr size_t OFF_STAGE = OFF_NS + (size_t)G::TM * 4;               // [WAVES][kFtMaxCap] uint2
  static constexpr size_t OFF_FLAG = OFF_STAGE + (size_t)G::WAVES * kFtMaxCap * 8;  // [2] i32
  static constexpr size_t LDS = OFF_FLAG + 16;
};

struct FtArg {
  const float* U;
  int64_t ldu, n_users;
  const float* I;
  int64_t ldi, n_items;
  const int64_t* users;  // nullable: query b is user b
  int64_t n_query;
  const int64_t* uptr;
  const int32_t* hist;
  uint2* cand;    // [nsplit][slots][cap]: x = score bits, y = item
  int32_t* ccnt;  // [nsplit][slots]: entries of each partial list (sorted, <= k)
  int64_t slots;  // query tiles * TM
  int64_t tiles_per_split;
  int k, cap;
};

template <int C>
__global__ void __launch_bounds__(FtCfg<C>::NT, 1) k_full_topk(FtArg a) {
  using F = FtCfg<C>;
  extern __shared__ __attribute__((aligned(16))) unsigned char ft_lds[];
  uint32_t* sMask = reinterpret_cast<uint32_t*>(ft_lds + F::OFF_MASK);
  int* sCnt = reinterpret_cast<int*>(ft_lds + F::OFF_CNT);
  float* sThr = reinterpret_cast<float*>(ft_lds + F::OFF_THR);
  int* sNs = reinterpret_cast<int*>(ft_lds + F::OFF_NS);  // entries kept in order by the last compaction
  int* sFlag = reinterpret_cast<int*>(ft_lds + F::OFF_FLAG);  // [tile parity]: a buffer ran full in the tile before
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  uint2* sStage = reinterpret_cast<uint2*>(ft_lds + F::OFF_STAGE) + wave * kFtMaxCap;
  const int64_t n_items = a.n_items, ldi = a.ldi;
  const int64_t ntiles = (n_items + F::TN - 1) / F::TN;
  const int64_t t0 = (int64_t)blockIdx.y * a.tiles_per_split;  // t0 < ntiles (launcher)
  const int64_t t1 = t0 + a.tiles_per_split < ntiles ? t0 + a.tiles_per_split : ntiles;
  const int64_t jlo = t0 * F::TN;
  const int64_t jhi = t1 * F::TN < n_items ? t1 * F::TN : n_items;
  const int k = a.k, cap = a.cap;

  // ---- this lane's query: user column r of the wave's 32; rows past n_query repeat the last ----
  const int wu = wave * 32 + r;
  const int64_t b = (int64_t)blockIdx.x * F::TM + wu;
  const int64_t bc = b < a.n_query ? b : a.n_query - 1;
  const int64_t u = clamp_idx(a.users ? a.users[bc] : bc, a.n_users);
  u32x4 ub[F::KS][3];
  score::load_owned<F>(a.U + u * a.ldu, hf, ub);
  // the block's candidate buffers: one of cap entries per query slot (b < slots always)
  uint2* const cblk = a.cand + ((int64_t)blockIdx.y * a.slots + (int64_t)blockIdx.x * F::TM) * cap;
  uint2* const cmine = cblk + (int64_t)wu * cap;

  // ---- the exclusion cursor of query tid (threads 0 .. TM-1) ----
  score::HistCursor cursor;
  if (tid < F::TM) {
    sCnt[tid] = 0;
    sThr[tid] = -INFINITY;
    sNs[tid] = 0;
    if (tid < 2) sFlag[tid] = 0;
    const int64_t be = (int64_t)blockIdx.x * F::TM + tid;
    if (be < a.n_query && a.uptr) cursor.seek(a.uptr, a.hist, clamp_idx(a.users ? a.users[be] : be, a.n_users), jlo);
  }
  cursor.start(a.hist);
  auto build_mask = [&](int64_t t, int bufi) {
    if (tid < F::TM) score::mask_words<F>(sMask + ((size_t)bufi * F::TM + tid) * F::SUB, t * F::TN, jhi, cursor, a.hist);
  };

  float4 pf[F::UPT][2];
  auto load_tile = [&](int64_t t) {
    score::tile_load<F>(pf, t, n_items, tid, [&](int64_t j) { return a.I + j * ldi; });
  };
  auto store_tile = [&](int bufi) { score::tile_store<F>(ft_lds + bufi * F::BUF, pf, tid); };

  // Compaction of user column ur of this wave (wave-uniform; all 64 lanes take part).  The buffer
  // holds ns entries in order (what the last compaction kept) and n - ns appended since.  All n are
  // staged in LDS and each lane places its <= 3 entries: position = entries that beat it = (for a
  // kept entry) its own index, (for an appended one) a binary search among the kept, plus, for
  // both, a count over the appended ones.  The first k are written back in order and thr becomes
  // the k-th.  Appends and compactions of one user's buffer are all by this wave.  The caller runs
  // ft_fence() once before a round of compactions, so that the appended entries (other lanes'
  // stores) have landed before they are loaded; inside a round the users' buffers are disjoint.
  auto compact = [&](int ur) {
    const int w2 = wave * 32 + ur;
    ft_fence_wave();
    const int n = *reinterpret_cast<volatile int*>(sCnt + w2);  // <= cap
    const int ns = *reinterpret_cast<volatile int*>(sNs + w2);  // <= min(n, k)
    uint2* gb = cblk + (int64_t)w2 * cap;
    uint2 mine[kFtPerLane];
    float ms[kFtPerLane];
    int rk[kFtPerLane];
#pragma unroll
    for (int i = 0; i < kFtPerLane; ++i) {
      const int e = lane + 64 * i;
      mine[i] = make_uint2(0u, 0u);
      if (e < n) {
        mine[i] = gb[e];
        sStage[e] = mine[i];
      }
      ms[i] = __uint_as_float(mine[i].x);
      rk[i] = e;
    }
    ft_fence_wave();  // every lane's loads have returned (their data went to LDS): the buffer may be rewritten
#pragma unroll
    for (int i = 0; i < kFtPerLane; ++i) {
      const int e = lane + 64 * i;
      if (e >= ns && e < n) {  // appended: the kept entries that beat it are a prefix of the kept
        int lo = 0, hi = ns;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          const uint2 o = sStage[mid];
          if (ft_beats(__uint_as_float(o.x), o.y, ms[i], mine[i].y)) lo = mid + 1; else hi = mid;
        }
        rk[i] = lo;
      }
    }
    for (int j = ns; j < n; ++j) {
      const uint2 o = sStage[j];
      const float os = __uint_as_float(o.x);
#pragma unroll
      for (int i = 0; i < kFtPerLane; ++i) rk[i] += ft_beats(os, o.y, ms[i], mine[i].y) ? 1 : 0;
    }
#pragma unroll
    for (int i = 0; i < kFtPerLane; ++i) {
      if (lane + 64 * i < n && rk[i] < k) {
        gb[rk[i]] = mine[i];
        if (rk[i] == k - 1) sThr[w2] = ms[i];
      }
    }
    if (lane == 0) {
      sCnt[w2] = n < k ? n : k;
      sNs[w2] = n < k ? n : k;
    }
    ft_fence_wave();
  };

  load_tile(t0);
  store_tile(0);
  build_mask(t0, 0);
  __syncthreads();

  float thr = -INFINITY;
  int cnt = 0;  // entries in the user's buffer: the same number in the user's two lanes
  const int xoff = F::xoff(r, hf);
  for (int64_t t = t0; t < t1; ++t) {
    const int bufi = (int)((t - t0) & 1);
    if (t + 1 < t1) load_tile(t + 1);
    // A compaction stalls its wave for microseconds, and through the tile barrier the block.  The
    // users of a block fill their buffers at about the same pace, so when one buffer ran full in
    // the tile before, every wave compacts now all its users that have kFtEarly or more appended
    // entries: the waves do that work at the same time instead of one after the other.  (When a
    // compaction happens never changes the result.)
    if (*reinterpret_cast<volatile int*>(sFlag + bufi)) {
      uint64_t want = __builtin_amdgcn_ballot_w64(cnt - *reinterpret_cast<volatile int*>(sNs + wu) >= kFtEarly);
      if (want) {
        if (hf == 0) sCnt[wu] = cnt;
        ft_fence();
        want = (want | (want >> 32)) & 0xffffffffull;
        while (want) {
          const int ur = __builtin_ctzll(want);
          want &= want - 1;
          compact(ur);
        }
        thr = *reinterpret_cast<volatile float*>(sThr + wu);
        cnt = *reinterpret_cast<volatile int*>(sCnt + wu);
      }
    }
    const unsigned char* tile_r = ft_lds + bufi * F::BUF + r * F::ROWB;
    u32x4 fa[3];
    score::read_a<F>(tile_r, 0, xoff, fa);
    f32x16 acc;
    // k_full_rank's flat (subtile, k step) sequence -- the next step's three A units read from LDS
    // while the current step's six MFMAs run, across the subtile boundary too -- written as two
    // nested loops so that the epilogue's code stands once per subtile in the unrolled body
#pragma unroll
    for (int sb = 0; sb < F::SUB; ++sb) {
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
      for (int ks = 0; ks < F::KS; ++ks) {
        const int idx = sb * F::KS + ks;
        u32x4 fn[3];
        if (idx + 1 < F::SUB * F::KS) score::read_a<F>(tile_r, idx + 1, xoff, fn);
        acc = mfma32_x6(fa, ub[ks], acc);
        __builtin_amdgcn_sched_barrier(0);
        if (idx + 1 < F::SUB * F::KS) {
          fa[0] = fn[0];
          fa[1] = fn[1];
          fa[2] = fn[2];
        }
      }
      // accumulator q of lane (r, hf) is item row acc_row(q) + 4 hf of user column r
      const uint32_t m = sMask[((size_t)bufi * F::TM + wu) * F::SUB + sb] >> (4 * hf);
      // the 16 pass predicates as wave masks (one compare each, the rest is scalar work); their
      // union decides the branch
      uint64_t bq[16], anyq = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        bq[q] = __builtin_amdgcn_ballot_w64(acc[q] > thr);
        anyq |= bq[q];
      }
      if (anyq == 0) continue;
      if (__builtin_amdgcn_ballot_w64(m != 0u) != 0) {  // some lane has excluded items in this subtile
        anyq = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          bq[q] &= __builtin_amdgcn_ballot_w64(((m >> score::acc_row(q)) & 1u) == 0u);
          anyq |= bq[q];
        }
        if (anyq == 0) continue;
      }
      // room for the 32 items of this subtile in every buffer of the wave
      uint64_t need = __builtin_amdgcn_ballot_w64(cnt + 32 > cap);
      if (need) {
        if (hf == 0) sCnt[wu] = cnt;
        ft_fence();
        if (lane == 0) sFlag[bufi ^ 1] = 1;
        need = (need | (need >> 32)) & 0xffffffffull;
        while (need) {
          const int ur = __builtin_ctzll(need);
          need &= need - 1;
          compact(ur);
        }
        thr = *reinterpret_cast<volatile float*>(sThr + wu);
        cnt = *reinterpret_cast<volatile int*>(sCnt + wu);
#pragma unroll
        for (int q = 0; q < 16; ++q) bq[q] &= __builtin_amdgcn_ballot_w64(acc[q] > thr);
      }
      // One accumulator register at a time, skipped when no lane passes in it (the usual case).  The
      // user's two lanes hold the same cnt and see each other's bit in the mask: hf = 0 takes slot
      // cnt, hf = 1 the one after it if both pass -- no atomic is needed.  (The item's row is
      // score::acc_row(q), kept as two summands: folded into one constant it compiles to 31-62 fewer
      // VGPRs at C <= 128 and to another nominal occupancy, a change to make with a measurement.)
      const int item0 = (int)(t * F::TN) + 32 * sb + 4 * hf;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        if (bq[q] == 0) continue;
        const int own = (int)((bq[q] >> lane) & 1u), oth = (int)((bq[q] >> (lane ^ 32)) & 1u);
        if (own) cmine[cnt + (hf & oth)] = make_uint2(__float_as_uint(acc[q]), (uint32_t)(item0 + (q & 3) + 8 * (q >> 2)));
        cnt += own + oth;
      }
    }
    if (t + 1 < t1) {
      store_tile(bufi ^ 1);
      build_mask(t + 1, bufi ^ 1);
    }
    if (tid == 0) sFlag[bufi] = 0;  // read at this tile's start; set again during the next tile at the earliest
    __syncthreads();
  }
  // every buffer sorted and cut to k: the split's partial list
  if (hf == 0) sCnt[wu] = cnt;
  ft_fence();
  for (int ur = 0; ur < 32; ++ur) compact(ur);
  ft_fence();
  if (hf == 0) a.ccnt[(int64_t)blockIdx.y * a.slots + b] = *reinterpret_cast<volatile int*>(sCnt + wu);
}

// One wave per query: the nsplit sorted partial lists (item ranges ascending with the split) merged
// under the total order, one list at a time against the running best k, by counting positions.
__global__ void __launch_bounds__(64) k_full_topk_merge(const uint2* cand, const int32_t* ccnt, int64_t slots, int cap,
                                                        int nsplit, int k, int32_t* out_idx, float* out_score) {
  __shared__ uint2 sL[2][2 * kFtMaxK];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  int cur = 0, nb = 0;
  if (nsplit == 1) {  // already the answer
    nb = ccnt[b];
    for (int e = lane; e < nb; e += 64) sL[0][e] = cand[b * cap + e];
    __syncthreads();
  }
  for (int y = 0; y < nsplit && nsplit > 1; ++y) {
    const int c = ccnt[(int64_t)y * slots + b];  // <= k
    const uint2* src = cand + ((int64_t)y * slots + b) * cap;
    for (int e = lane; e < c; e += 64) sL[cur][nb + e] = src[e];
    __syncthreads();
    const int n = nb + c;  // <= 2 k
    for (int e = lane; e < n; e += 64) {
      const uint2 me = sL[cur][e];
      const float ms = __uint_as_float(me.x);
      int rk = 0;
      for (int j = 0; j < n; ++j) {
        const uint2 o = sL[cur][j];
        rk += ft_beats(__uint_as_float(o.x), o.y, ms, me.y) ? 1 : 0;
      }
      if (rk < k) sL[cur ^ 1][rk] = me;
    }
    __syncthreads();
    nb = n < k ? n : k;
    cur ^= 1;
  }
  for (int e = lane; e < k; e += 64) {
    const uint2 v = sL[cur][e < nb ? e : 0];
    out_idx[b * k + e] = e < nb ? (int32_t)v.y : -1;
    if (out_score) out_score[b * k + e] = e < nb ? __uint_as_float(v.x) : -INFINITY;
  }
}

struct FtPlan {
  int64_t utiles, nsplit, tiles_per_split, slots;
  int cap;
  size_t cnt_off, bytes;
};

// room for the 32 items of a subtile on top of k kept entries, and 32 more so that two compactions
// of a full buffer are at least 33 appends apart
int ft_cap(int k) { return (k + 64 + 31) / 32 * 32; }
static_assert((kFtMaxK + 64 + 31) / 32 * 32 == kFtMaxCap, "the LDS staging area holds the largest buffer");

template <int C>
FtPlan ft_plan(int64_t n_query, int64_t n_items, int k, int ncu) {
  using F = FtCfg<C>;
  FtPlan p;
  p.utiles = (n_query + F::TM - 1) / F::TM;
  // too few query tiles to fill the chip: the item range is split
  const score::ItemSplit sp = score::split_items(p.utiles, (n_items + F::TN - 1) / F::TN, ncu);
  p.nsplit = sp.nsplit;
  p.tiles_per_split = sp.tiles_per_split;
  p.slots = p.utiles * F::TM;
  p.cap = ft_cap(k);
  p.cnt_off = (size_t)p.nsplit * p.slots * p.cap * sizeof(uint2);
  p.bytes = (p.cnt_off + (size_t)p.nsplit * p.slots * sizeof(int32_t) + 255) / 256 * 256;
  return p;
}

FtPlan ft_plan_any(int C, int64_t n_query, int64_t n_items, int k, int ncu) {
  switch (C) {
    case 32: return ft_plan<32>(n_query, n_items, k, ncu);
    case 64: return ft_plan<64>(n_query, n_items, k, ncu);
    case 128: return ft_plan<128>(n_query, n_items, k, ncu);
    default: return ft_plan<256>(n_query, n_items, k, ncu);
  }
}

template <int C>
hipError_t launch_full_topk(FtArg a, const FtPlan& p, hipStream_t st) {
  using F = FtCfg<C>;
  const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_full_topk<C>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)F::LDS);
  if (attr != hipSuccess) return attr;
  if (p.utiles > 0x7fffffff || p.nsplit > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_full_topk<C>, dim3((unsigned)p.utiles, (unsigned)p.nsplit), dim3(F::NT), F::LDS, st, a);
  return hipGetLastError();
}

}  // namespace

bool full_topk_channels_ok(int C) { return C == 32 || C == 64 || C == 128 || C == 256; }
int full_topk_max_k() { return kFtMaxK; }

size_t full_topk_workspace_floor(int64_t n_query, int64_t n_items, int C, int k) {
  return n_query > 0 ? ft_plan_any(C, n_query, n_items, k, 1).bytes : 0;
}

hipError_t full_topk_workspace(int64_t n_query, int64_t n_items, int C, int k, size_t* bytes) {
  *bytes = 0;
  if (n_query == 0) return hipSuccess;
  int ncu = 0;
  const hipError_t e = score::cu_count(&ncu);
  if (e != hipSuccess) return e;
  *bytes = ft_plan_any(C, n_query, n_items, k, ncu).bytes;
  return hipSuccess;
}

hipError_t full_topk(const float* U, int64_t ldu, int64_t n_users, const float* I, int64_t ldi, int64_t n_items, int C,
                     const int64_t* users, int64_t n_query, const int64_t* uptr, const int32_t* hist, int k,
                     int32_t* out_idx, float* out_score, void* ws, size_t ws_bytes, hipStream_t st) {
  if (n_query == 0) return hipSuccess;
  if (n_query > 0x7fffffff) return hipErrorInvalidValue;  // one merge block per query
  int ncu = 0;
  hipError_t e = score::cu_count(&ncu);
  if (e != hipSuccess) return e;
  const FtPlan p = ft_plan_any(C, n_query, n_items, k, ncu);
  if (!ws || ws_bytes < p.bytes) return hipErrorInvalidValue;
  uint2* cand = static_cast<uint2*>(ws);
  int32_t* ccnt = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(ws) + p.cnt_off);
  FtArg a{U, ldu, n_users, I, ldi, n_items, users, n_query, uptr, hist, cand, ccnt, p.slots, p.tiles_per_split, k, p.cap};
  switch (C) {
    case 32: e = launch_full_topk<32>(a, p, st); break;
    case 64: e = launch_full_topk<64>(a, p, st); break;
    case 128: e = launch_full_topk<128>(a, p, st); break;
    case 256: e = launch_full_topk<256>(a, p, st); break;
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_full_topk_merge, dim3((unsigned)n_query), dim3(64), 0, st, cand, ccnt, p.slots, p.cap, (int)p.nsplit,
                     k, out_idx, out_score);
  return hipGetLastError();
}

}  // namespace ppgat
