// Replay movers: pool rows <-> batch rows for every key of a replay in one launch
// (gather: Replay.sample, scatter: Replay.add / Replay.update), flat and span
// forms, arguments by value, staged through LDS or read through a pointer.
#include "device_util.h"
#include "knobs.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>

namespace emb {
namespace {

// What a persistent span-mover workgroup needs before its first load, in one
// contiguous 160-byte block at the very start of the arguments: a wave copies
// it into registers with three independent scalar loads (one memory latency)
// instead of walking four or five dependent ones through the full plan — which
// matters most when the plan is read through a pointer (host-resident kernel
// arguments: the device copy starts out cold in every XCD's L2).
constexpr int kSpanKeys = 4;     // wide keys per span launch (more: flat mover)
struct alignas(16) SpanHead {
  int32_t wide_workers, n_wide, seq_len, group;
  int64_t group_stride;
  uint32_t ntiles, pad_;
  uint32_t tile0[kSpanKeys];          // first tile of wide key k; 0xFFFFFFFF beyond n_wide
  uint32_t tiles_per_seq[kSpanKeys];
  // 16-byte units of one sequence of wide key k on the batch side: its head
  // length (MovePlan::key_len, seq_len unless the key is a context-only one)
  // times rowbytes / 16.
  uint32_t units_per_seq[kSpanKeys];
  KeyDesc key[kSpanKeys];
};
static_assert(sizeof(SpanHead) == 176, "SpanHead is loaded as 44 dwords");

// Per-launch plan in kernel-argument memory (< 4 KiB).
// Everything of a launch plan except the head and the inline words: which key
// owns which virtual blocks, the keys themselves, how rows are resolved.  One
// contiguous block so that the by-value movers can bring it into LDS with one
// load per lane when the arguments live in host memory (see stage_tables).
struct alignas(16) MoveTables {
  KeyDesc key[kMaxKeys];
  int32_t first_block[kMaxKeys + 1];
  int32_t unit[kMaxKeys];           // 0: 16-byte flat path; else bytes per lane
  // Steps of a sequence that key k moves (its head: seq_len, or fewer for a
  // context-only key of a gather) and its batch rows in this launch
  // (n_seq * key_len[k]; n_rows when every key moves whole sequences).
  int32_t key_len[kMaxKeys];
  int32_t key_rows[kMaxKeys];
  int32_t n_keys, n_rows, seq_len, key_is_first, key_is_last;
  int32_t rows_mode;                // 0 device table, 1 inline rows, 2 inline spans
  int32_t inline_key, inline_key_word0;
  const uint8_t* is_first_pool;
  const int32_t* rows;
  uint32_t mask_bits;               // scatter: keys written as value * !mask_flags[r]
  int8_t mask_dtype[kMaxKeys];
  uint8_t* mask_out[kMaxKeys];
  const uint8_t* mask_flags;
  // The batch side in groups of `group` sequences, `group_stride` bytes apart
  // (0 = one dense (n_rows, rowbytes) array per key).  Sequence s of key k
  // starts at key.batch + (s / group) * group_stride + (s % group) * L *
  // rowbytes: the layout of a packed batch cut into per-destination-rank blocks
  // (distributed.py, DP-slice exchange), written by a grouped gather and read
  // by a grouped write-back (emb_replay_update_grouped).
  int32_t group;
  int64_t group_stride;
};
static_assert(sizeof(MoveTables) % 16 == 0 && sizeof(MoveTables) / 16 <= 64,
              "the tables are staged as one 16-byte load per lane of one wave");

// Per-launch plan in kernel-argument memory (< 4 KiB).  Span mode (rows_mode 2):
// the wide keys are moved by `head.wide_workers` persistent workgroups walking
// `head.ntiles` tiles (see move_wide_spans); those keys own no virtual blocks.
struct alignas(16) MoveArgs {
  SpanHead head;
  // Row table / span table / step ids carried in the arguments.  Directly behind
  // the head: the span mover stages head + the first spans with ONE load per lane.
  uint32_t inline_words[kInlineWords];
  MoveTables t;
};
static_assert(sizeof(MoveArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// What the span mover stages through LDS before anything else: the head and the
// first spans, contiguous in the arguments.
constexpr int kStagedSeqs = 70;      // (176 + 70 * 12 + 8) / 16 = 64 lanes: one wave, one load each
struct StagedSpans {
  SpanHead head;
  uint32_t spans[3 * kStagedSeqs];
  uint32_t tail_[2];                  // (two words of span 70: never read from here)
};
static_assert(sizeof(StagedSpans) == 64 * 16, "one 16-byte load per lane of one wave");
static_assert(offsetof(MoveArgs, inline_words) == sizeof(SpanHead), "spans follow the head");


__device__ __forceinline__ int find_key(const MoveTables& tb, int block) {
  int k = 0;
  while (k + 1 < tb.n_keys && block >= tb.first_block[k + 1]) ++k;
  return k;
}

// Pool row of step t of sequence seq.  (A launch's row table is n_seq
// sequences of tb.seq_len steps; a key's batch side holds the first klen of
// them, so batch row r of that key is (seq, t) = (r / klen, r % klen).)
// kLds: the launch's first kFlatStagedSeqs spans were staged into LDS (`lds`)
// together with the tables -- the indirect flat movers, whose argument block
// lives in uncached device memory (see flat_move_kernel_indirect).
constexpr int kFlatStagedSeqs = 64;      // 192 words = 48 lanes, one 16-byte load each
template <bool kLds = false>
__device__ __forceinline__ int32_t row_at(const MoveArgs& a, const MoveTables& tb, uint32_t seq, uint32_t t,
                                          const uint32_t* lds = nullptr) {
  if (tb.rows_mode == 2) {
    if (kLds && seq < static_cast<uint32_t>(kFlatStagedSeqs)) {
      const uint32_t row0 = lds[3 * seq], n0 = lds[3 * seq + 1];
      return static_cast<int32_t>(t < n0 ? row0 + t : lds[3 * seq + 2] + (t - n0));
    }
    const uint32_t row0 = a.inline_words[3 * seq], n0 = a.inline_words[3 * seq + 1];
    return static_cast<int32_t>(t < n0 ? row0 + t : a.inline_words[3 * seq + 2] + (t - n0));
  }
  const uint32_t r = seq * static_cast<uint32_t>(tb.seq_len) + t;
  if (tb.rows_mode == 1) return static_cast<int32_t>(a.inline_words[r]);
  return tb.rows[r];
}

// Byte offset of step t of sequence seq of `key` on the batch side (klen steps
// per sequence there; see MoveArgs::group).
__device__ __forceinline__ int64_t batch_offset(const MoveTables& tb, const KeyDesc& key, uint32_t klen,
                                                uint32_t seq, uint32_t t) {
  if (tb.group == 0) return static_cast<int64_t>(seq * klen + t) * key.rowbytes;
  const uint32_t g = static_cast<uint32_t>(tb.group);
  const uint32_t grp = seq / g, j = seq - grp * g;
  return static_cast<int64_t>(grp) * tb.group_stride + static_cast<int64_t>(j * klen + t) * key.rowbytes;
}

// A key's rows are moved as a flat sequence of 16-byte units: unit u belongs to
// batch row u / upr.  A workgroup owns blockDim.x * U consecutive units; lane j
// takes units j, j + blockDim.x, ...: consecutive lanes touch consecutive
// 16 bytes on both sides, every lane has U independent row lookups and then U
// independent loads in flight before its first store, and no lane waits on a
// per-workgroup scalar dependency chain.
template <bool kGather, int U, int NT, bool kLds = false>
__device__ __forceinline__ void move_wide(const MoveArgs& a, const MoveTables& tb, const KeyDesc& key, int k,
                                          int local, const uint32_t* lds = nullptr) {
  const uint32_t upr = static_cast<uint32_t>(key.rowbytes >> 4);
  const uint32_t klen = static_cast<uint32_t>(tb.key_len[k]);
  const uint32_t nrows = static_cast<uint32_t>(tb.key_rows[k]);
  const uint32_t total = upr * nrows;
  // (Workgroup b runs on XCD b % 8 and takes tile b: every frame is spread over
  // all XCDs' memory channels, which a streaming copy prefers -- giving each XCD
  // one contiguous eighth of the batch instead measured 2-3 % slower.)
  // One division per wave for the workgroup's first unit; lanes step from it
  // with adds and compares (a 32-bit divide costs ~40 VALU instructions).
  const uint32_t base = static_cast<uint32_t>(local) * (blockDim.x * U);
  const uint32_t r0 = base / upr;
  const uint32_t off0 = base - r0 * upr;
  const uint32_t seq0 = r0 / klen, t0 = r0 - seq0 * klen;
  // The workgroup's units span at most kRows consecutive batch rows when rows
  // are long (the usual case: one 28 KB frame = 1764 units): resolve those rows
  // ONCE per wave with wave-uniform (scalar) reads of the inline span table and
  // let the lanes select, instead of every lane reading the table.
  constexpr int kRows = 3;
  const bool few_rows = tb.rows_mode == 2 &&
                        (off0 + blockDim.x * U - 1) / upr < static_cast<uint32_t>(kRows);
  int32_t row_tab[kRows];
  if (few_rows) {
    uint32_t seq = seq0, t = t0;
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      // (rows_mode 2 spelled out, not row_at: its other modes read through
      // tb.rows, and a wave-uniform choice between that pointer and one into the
      // by-value argument block makes the compiler copy the whole block -- 3.8 KB
      // per lane -- to scratch)
      if (r0 + i < nrows) {
        if (kLds && seq < static_cast<uint32_t>(kFlatStagedSeqs)) {
          const uint32_t start = lds[3 * seq], n0 = lds[3 * seq + 1];
          row_tab[i] = static_cast<int32_t>(t < n0 ? start + t : lds[3 * seq + 2] + (t - n0));
        } else {
          const uint32_t start = a.inline_words[3 * seq], n0 = a.inline_words[3 * seq + 1];
          row_tab[i] = static_cast<int32_t>(t < n0 ? start + t : a.inline_words[3 * seq + 2] + (t - n0));
        }
      } else {
        row_tab[i] = -1;
      }
      if (++t >= klen) { t = 0; ++seq; }
    }
  }
  uint32_t sq[U], tt[U], off[U];
  int32_t row[U];
#pragma unroll
  for (int j = 0; j < U; ++j) {
    uint32_t x = off0 + j * blockDim.x + threadIdx.x, dr = 0;
    while (x >= upr) { x -= upr; ++dr; }
    uint32_t seq = seq0, t = t0 + dr;
    while (t >= klen) { t -= klen; ++seq; }
    sq[j] = seq;
    tt[j] = t;
    off[j] = x;
    if (base + j * blockDim.x + threadIdx.x >= total) {
      row[j] = -1;
    } else if (few_rows) {
      row[j] = dr == 0 ? row_tab[0] : dr == 1 ? row_tab[1] : row_tab[2];
    } else {
      row[j] = row_at<kLds>(a, tb, seq, t, lds);
    }
  }
  u32x4 buf[U];
#pragma unroll
  for (int j = 0; j < U; ++j) {
    if (row[j] < 0) continue;
    const uint8_t* pool = key.pool + static_cast<int64_t>(row[j]) * key.rowbytes;
    const uint8_t* batch = key.batch + batch_offset(tb, key, klen, sq[j], tt[j]);
    const u32x4* src = reinterpret_cast<const u32x4*>(kGather ? pool : batch) + off[j];
    buf[j] = load16<(NT & 1) != 0>(src);
  }
#pragma unroll
  for (int j = 0; j < U; ++j) {
    if (row[j] < 0) continue;
    uint8_t* pool = key.pool + static_cast<int64_t>(row[j]) * key.rowbytes;
    uint8_t* batch = key.batch + batch_offset(tb, key, klen, sq[j], tt[j]);
    u32x4* dst = reinterpret_cast<u32x4*>(kGather ? batch : pool) + off[j];
    store16<(NT & 2) != 0>(dst, buf[j]);
  }
}

// Span mode: every sequence is one or two contiguous runs of pool rows
// ({row0, n0, row1}: rows row0..row0+n0-1, then row1..), so per wide key a
// sequence is a flat run of L * rowbytes/16 units with ONE split point and no
// row structure at all.  `wide_workers` workgroups (a couple per CU) walk the
// tiles of blockDim.x * U units with a grid stride, and every lane issues the
// NEXT tile's loads before it stores the current one: loads and stores of one
// workgroup overlap and the launch has a single ramp instead of one per
// 8 KB workgroup.  Measured on MI355X (tools/gather_lab.hip, B=16, L=65,
// 28 224-byte rows, cold 2.8 GB pool): 10.0-10.2 us against 10.1 us for a
// plain contiguous copy of the same bytes and 13.8 us for the flat
// one-tile-per-workgroup mover above.
template <bool kGather, int U, int NT>
__device__ __forceinline__ void move_wide_spans(const MoveArgs& a, const StagedSpans& staged) {
  const SpanHead& h = staged.head;
  const uint32_t tile = blockDim.x * U;
  const uint32_t ntiles = h.ntiles;
  const uint32_t stride = static_cast<uint32_t>(h.wide_workers);
  struct Where {
    const u32x4* p0; const u32x4* p1;   // pool runs, both indexed by the unit number
    const u32x4* b;                     // batch side of the sequence
    uint32_t split, total, u0;
  };
  auto locate = [&](uint32_t ti) {
    // Which wide key: tile0[] beyond n_wide is 0xFFFFFFFF.
    const int k = (ti >= h.tile0[1]) + (ti >= h.tile0[2]) + (ti >= h.tile0[3]);
    const KeyDesc key = h.key[k];
    const uint32_t tps = h.tiles_per_seq[k];
    const uint32_t local = ti - h.tile0[k];
    const uint32_t seq = local / tps, piece = local - seq * tps;
    const uint32_t upr = static_cast<uint32_t>(key.rowbytes >> 4);
    // The first kStagedSeqs spans came with the head (LDS); later ones are read
    // from the argument block.
    // (No pointer into `a` here: a by-value argument block whose address
    // escapes is copied to scratch, 3.7 KB per lane.)
    uint32_t row0, n0, row1;
    if (seq < kStagedSeqs) {
      row0 = staged.spans[3 * seq], n0 = staged.spans[3 * seq + 1], row1 = staged.spans[3 * seq + 2];
    } else {
      row0 = a.inline_words[3 * seq], n0 = a.inline_words[3 * seq + 1], row1 = a.inline_words[3 * seq + 2];
    }
    Where w;
    w.split = n0 * upr;
    w.total = h.units_per_seq[k];     // (a context-only key: fewer than L * upr, all of them maybe left of the split)
    w.u0 = piece * tile + threadIdx.x;
    w.p0 = reinterpret_cast<const u32x4*>(key.pool) + static_cast<uint64_t>(row0) * upr;
    w.p1 = reinterpret_cast<const u32x4*>(key.pool) + static_cast<uint64_t>(row1) * upr - w.split;
    if (h.group == 0) {
      w.b = reinterpret_cast<const u32x4*>(key.batch) + static_cast<uint64_t>(seq) * w.total;
    } else {
      const uint32_t g = static_cast<uint32_t>(h.group), grp = seq / g, j = seq - grp * g;
      w.b = reinterpret_cast<const u32x4*>(key.batch + static_cast<int64_t>(grp) * h.group_stride) +
            static_cast<uint64_t>(j) * w.total;
    }
    return w;
  };
  auto issue = [&](const Where& w, u32x4* v) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const uint32_t u = w.u0 + j * blockDim.x;
      if (u < w.total) {
        const u32x4* src = kGather ? (u < w.split ? w.p0 : w.p1) + u : w.b + u;
        v[j] = load16<(NT & 1) != 0>(src);
      }
    }
  };
  auto put = [&](const Where& w, const u32x4* v) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const uint32_t u = w.u0 + j * blockDim.x;
      if (u < w.total) {
        u32x4* dst = const_cast<u32x4*>(kGather ? w.b + u : (u < w.split ? w.p0 : w.p1) + u);
        store16<(NT & 2) != 0>(dst, v[j]);
      }
    }
  };
  uint32_t i = blockIdx.x;
  if (i >= ntiles) return;
  u32x4 cur[U], nxt[U];
  Where wc = locate(i);
  issue(wc, cur);
  for (;;) {
    const uint32_t n = i + stride;
    Where wn = wc;
    if (n < ntiles) {
      wn = locate(n);
      issue(wn, nxt);
    }
    put(wc, cur);
    if (n >= ntiles) break;
#pragma unroll
    for (int j = 0; j < U; ++j) cur[j] = nxt[j];
    wc = wn;
    i = n;
  }
}

// pool[rows[r]] -> batch[r] for every key of the replay in ONE launch, with
// the is_first / is_last annotation of replay.py:277-292 applied in flight.
template <int U, int NT, bool kLds = false>
__device__ __forceinline__ void gather_block(const MoveArgs& a, const MoveTables& tb, int block,
                                             const uint32_t* lds = nullptr) {
  const int k = find_key(tb, block);
  const KeyDesc key = tb.key[k];
  const int local = block - tb.first_block[k];
  const int unit = tb.unit[k];
  if (unit == 0) {
    move_wide<true, U, NT, kLds>(a, tb, key, k, local, lds);
    return;
  }
  const uint32_t klen = static_cast<uint32_t>(tb.key_len[k]);
  const int64_t upr = key.rowbytes / unit;
  const int64_t u = static_cast<int64_t>(local) * blockDim.x + threadIdx.x;
  if (u >= upr * tb.key_rows[k]) return;
  const int64_t r = u / upr;
  const int64_t off = (u - r * upr) * unit;
  const uint32_t seq = static_cast<uint32_t>(r) / klen, t = static_cast<uint32_t>(r) - seq * klen;
  const int64_t row = row_at<kLds>(a, tb, seq, t, lds);
  if (row < 0) return;   // not this rank's sequence (sharded pools): leave as is
  const uint8_t* src = key.pool + row * key.rowbytes + off;
  uint8_t* dst = key.batch + batch_offset(tb, key, klen, seq, t) + off;
  if (key.rowbytes == 1 && (k == tb.key_is_first || k == tb.key_is_last)) {
    // (annotated over the FULL sequence, then cut to the key's head: what
    // slicing the reference's annotated batch gives)
    uint8_t v = gload<uint8_t>(src);
    if (k == tb.key_is_first) {
      if (t == 0) v = 1;
    } else if (tb.is_first_pool && t + 1 < static_cast<uint32_t>(tb.seq_len)) {
      v |= gload<uint8_t>(tb.is_first_pool + row_at<kLds>(a, tb, seq, t + 1, lds));
    }
    gstore<uint8_t>(dst, v);
    return;
  }
  copy_bytes(src, dst, unit);
}

template <bool kLds = false>
__device__ __forceinline__ void scatter_masked(const MoveArgs& a, const MoveTables& tb, int k, const KeyDesc& key, int local,
                                               const uint32_t* lds = nullptr) {
  const int es = tb.unit[k];                       // element size of the key's dtype
  const int64_t epr = key.rowbytes / es;
  const int64_t e = static_cast<int64_t>(local) * blockDim.x + threadIdx.x;
  if (e >= epr * tb.n_rows) return;
  const int64_t r = e / epr;
  const int64_t off = (e - r * epr) * es;
  const uint32_t L = static_cast<uint32_t>(tb.seq_len), seq = static_cast<uint32_t>(r) / L;
  const int64_t row = row_at<kLds>(a, tb, seq, static_cast<uint32_t>(r) - seq * L, lds);
  const bool keep = gload<uint8_t>(tb.mask_flags + r) == 0;
  const uint8_t* src = key.batch + r * key.rowbytes + off;
  uint8_t* pool = row >= 0 ? key.pool + row * key.rowbytes + off : nullptr;
  uint8_t* out = tb.mask_out[k] ? tb.mask_out[k] + r * key.rowbytes + off : nullptr;
  put_masked_as(tb.mask_dtype[k], src, pool, out, keep);
}

// batch[r] -> pool[rows[r]]; rows[r] < 0 are skipped (evicted update targets).
template <int U, int NT, bool kLds = false>
__device__ __forceinline__ void scatter_block(const MoveArgs& a, const MoveTables& tb, int block,
                                              const uint32_t* lds = nullptr) {
  const int k = find_key(tb, block);
  const KeyDesc key = tb.key[k];
  const int local = block - tb.first_block[k];
  const int unit = tb.unit[k];
  if ((tb.mask_bits >> k) & 1u) {
    scatter_masked<kLds>(a, tb, k, key, local, lds);
    return;
  }
  if (unit == 0) {
    move_wide<false, U, NT, kLds>(a, tb, key, k, local, lds);
    return;
  }
  const int64_t upr = key.rowbytes / unit;
  const int64_t u = static_cast<int64_t>(local) * blockDim.x + threadIdx.x;
  if (u >= upr * tb.n_rows) return;
  const int64_t r = u / upr;
  const int64_t off = (u - r * upr) * unit;
  const uint32_t L = static_cast<uint32_t>(tb.seq_len), seq = static_cast<uint32_t>(r) / L;
  const int64_t row = row_at<kLds>(a, tb, seq, static_cast<uint32_t>(r) - seq * L, lds);
  if (row < 0) return;
  if (k == tb.inline_key) {   // batch bytes of this key ride in the kernel arguments
    const uint32_t w = a.inline_words[tb.inline_key_word0 + r * (key.rowbytes >> 2) + (off >> 2)];
    gstore<uint32_t>(key.pool + row * key.rowbytes + off, w);
    return;
  }
  // (grouped sources: batch_offset; a write-back moves whole sequences, klen = L)
  const int64_t src = tb.group == 0 ? r * key.rowbytes
                                    : batch_offset(tb, key, L, seq, static_cast<uint32_t>(r) - seq * L);
  copy_bytes(key.batch + src + off, key.pool + row * key.rowbytes + off, unit);
}

// A flat launch has first_block[n_keys] virtual blocks and exactly that many
// workgroups.  (A grid capped at a few workgroups per CU that walks the virtual
// blocks with a stride measured equal at B=16 and 7-8 % slower at B=64/256: the
// dispatcher overlaps one workgroup's stores with the next one's loads better.)
constexpr int kFlatUnroll = 2;      // 16-byte units per lane: 2 beats 4/8 by 10-15 % (MI355X sweep)
constexpr int kFlatNT = 3;          // non-temporal loads and stores: ~3 % faster than plain on cold lines
constexpr int kFlatThreads = 256;   // 64..512 within noise, 1024 slower

// The kernel-argument segment as raw 16-byte units (MoveArgs is the only
// parameter of every mover, so it starts the segment).  Indexing the by-value
// parameter itself with a lane id would make the compiler copy the whole
// 3.7 KB struct into scratch, per lane (260 us instead of 11).
__device__ __forceinline__ const u32x4* kernarg_units() {
  return (const u32x4*)(const __attribute__((address_space(4))) void*)__builtin_amdgcn_kernarg_segment_ptr();
}

// Host-resident kernel arguments: every scalar read of the plan is a PCIe round
// trip, and a flat-mover wave makes three or four dependent ones (which key is
// mine -> its descriptor -> my rows) before its first payload load.  The staged
// variants bring the tables into LDS with one 16-byte load per lane of the first
// wave: one round trip, then LDS reads; only the inline row words still come from
// the argument block.  (Insert scatter of 64 rows: 13.5 -> ~9 us.)
__device__ __forceinline__ void stage_tables(const u32x4* bytes, MoveTables* dst) {
  constexpr uint32_t first = offsetof(MoveArgs, t) / 16;
  if (threadIdx.x < sizeof(MoveTables) / 16)
    reinterpret_cast<u32x4*>(dst)[threadIdx.x] = bytes[first + threadIdx.x];
  __syncthreads();
}
static_assert(offsetof(MoveArgs, t) % 16 == 0, "the tables are staged in 16-byte units");

// Each mover exists three times: arguments by value in the kernel-argument
// segment (default), the same with the tables staged through LDS (arguments in
// host memory, small launches), or read through a pointer to a copy in device
// memory (arguments in host memory, big launches: abi.cpp run_move).
template <bool kGather, bool kLds = false>
__device__ __forceinline__ void flat_block(const MoveArgs& a, const MoveTables& tb, const uint32_t* lds = nullptr) {
  if (kGather) gather_block<kFlatUnroll, kFlatNT, kLds>(a, tb, blockIdx.x, lds);
  else scatter_block<kFlatUnroll, kFlatNT, kLds>(a, tb, blockIdx.x, lds);
}
template <bool kGather>
__global__ __launch_bounds__(kFlatThreads) void flat_move_kernel(const MoveArgs a) { flat_block<kGather>(a, a.t); }
template <bool kGather>
__global__ __launch_bounds__(kFlatThreads) void flat_move_kernel_staged(const MoveArgs a) {
  __shared__ MoveTables tables;
  stage_tables(kernarg_units(), &tables);
  flat_block<kGather>(a, tables);
}
// The device copy of the argument block sits in a ring of fine-grained (uncached)
// memory the CPU wrote through the BAR: every read of it goes to memory.  The
// tables AND the first kFlatStagedSeqs spans therefore come into LDS with one
// 16-byte load per lane -- wave 0 the tables, wave 1 the spans, both in flight
// together: one latency per workgroup, where a wave's scalar reads of its spans
// were a second, dependent one in front of every payload load (an 85 MB
// write-back through this mover: 20.3 us before, 17.1 us now; the by-value mover
// with device-resident arguments takes 13 us).
static_assert(kFlatThreads >= 64 + 3 * kFlatStagedSeqs / 4, "wave 1 stages the spans");
static_assert(3 * kFlatStagedSeqs <= kInlineWords && sizeof(SpanHead) % 16 == 0, "the staged spans lie inside the block");
template <bool kGather>
__global__ __launch_bounds__(kFlatThreads) void flat_move_kernel_indirect(const MoveArgs* __restrict__ a) {
  __shared__ MoveTables tables;     // one load latency instead of a chain of scalar loads
  __shared__ __attribute__((aligned(16))) uint32_t spans[3 * kFlatStagedSeqs];
  const u32x4* bytes = reinterpret_cast<const u32x4*>(a);
  constexpr uint32_t first_table = offsetof(MoveArgs, t) / 16, first_span = sizeof(SpanHead) / 16;
  if (threadIdx.x < sizeof(MoveTables) / 16)
    reinterpret_cast<u32x4*>(&tables)[threadIdx.x] = bytes[first_table + threadIdx.x];
  else if (threadIdx.x >= 64 && threadIdx.x < 64 + 3 * kFlatStagedSeqs / 4)
    reinterpret_cast<u32x4*>(spans)[threadIdx.x - 64] = bytes[first_span + threadIdx.x - 64];
  __syncthreads();
  flat_block<kGather, true>(*a, tables, spans);
}

// Span-mode launch: the first `wide_workers` workgroups are the persistent wide
// movers, the rest are the virtual blocks of the narrow keys.
// The 160-byte head goes from the argument block to LDS with one 16-byte load
// per lane of the first ten lanes — a single memory latency however the
// compiler would have scheduled the individual field reads.
// `bytes`: the argument block as raw 16-byte units — the device copy for the
// indirect kernels, the kernel-argument segment itself for the by-value ones.
__device__ __forceinline__ void stage_head(const u32x4* bytes, StagedSpans* dst) {
  if (threadIdx.x < sizeof(StagedSpans) / 16)
    reinterpret_cast<u32x4*>(dst)[threadIdx.x] = bytes[threadIdx.x];
  __syncthreads();
}

// Shape of the persistent mover (MI355X, profiles/r04_gather_shapes.txt and
// r04_ab_span_shape.txt): 256 threads x 4 units per lane = tiles of 16 KB, four
// workgroups per CU, every worker slot filled -- B=16 10.1-10.3 us against
// 10.8-11.2 for 512 threads x 2 per CU; U=2 and 1024-thread shapes were slower.
constexpr int kSpanUnroll = 4;
constexpr int kSpanThreads = 256;
constexpr int kSpanPerCU = 4;
template <bool kGather, int NT>
__device__ __forceinline__ void span_move_body(const MoveArgs& a, const u32x4* bytes) {
  __shared__ StagedSpans staged;
  stage_head(bytes, &staged);
  if (static_cast<int>(blockIdx.x) < staged.head.wide_workers) {
    move_wide_spans<kGather, kSpanUnroll, NT>(a, staged);
    return;
  }
  const int block = static_cast<int>(blockIdx.x) - staged.head.wide_workers;
  if (kGather) gather_block<kFlatUnroll, NT>(a, a.t, block);
  else scatter_block<kFlatUnroll, NT>(a, a.t, block);
}

// NT: non-temporal hints, bit 0 loads, bit 1 stores.  3 (both) is the fastest
// gather by itself (B=16: 10.7 us against 11.2 / 10.9 / 12.2 for loads-only /
// stores-only / none); 1 (plain stores) leaves the batch in L2 / Infinity Cache
// for a reader that follows at once (EMB_GATHER_STORES=plain).
template <bool kGather, int NT>
__global__ __launch_bounds__(kSpanThreads) void span_move_kernel(const MoveArgs a) {
  // MoveArgs is the only parameter: it starts the kernel-argument segment.
  span_move_body<kGather, NT>(a, kernarg_units());
}
template <bool kGather, int NT>
__global__ __launch_bounds__(kSpanThreads) void span_move_kernel_indirect(const MoveArgs* __restrict__ a) {
  span_move_body<kGather, NT>(*a, reinterpret_cast<const u32x4*>(a));
}

// Host-resident kernel arguments (HIP_FORCE_DEV_KERNARG=0): one workgroup
// copies the mover's argument block from the kernel-argument segment into
// device memory, so that the mover's thousands of waves read it from L2
// instead of each crossing PCIe.
// One 16-byte load per lane: the whole block crosses PCIe in a single round
// trip (word-sized loads took four, ~10 us).
__global__ __launch_bounds__(256) void args_writer_kernel(const MoveArgs a, u32x4* __restrict__ dst) {
  const u32x4* src = reinterpret_cast<const u32x4*>(&a);
  for (uint32_t i = threadIdx.x; i < sizeof(MoveArgs) / 16; i += blockDim.x) dst[i] = src[i];
}
static_assert(sizeof(MoveArgs) % 16 == 0 && sizeof(MoveArgs) / 16 <= 256,
              "argument block is copied as one dwordx4 per lane");

__global__ void marker_kernel() {}

// Which mover a launch gets (prepare_move).  The persistent span mover wins
// clearly while the launch is ramp-dominated and stays level with the flat
// mover's many short-lived workgroups far beyond that (MI355X, S0 rows, kernel us
// persistent / flat: B=8 6.8 / 8.7, B=16 10.7 / 13.4, B=32 22.5 / 23.5, B=64
// 41.7 / 42.1, B=128 81.6 / 79.4; Dreamer keys, 144 MB: 26.8 / 28.7), so gathers
// use it up to kSpanGatherMB of wide payload per launch.  Write-backs up to
// kSpanScatterMB: the flat scatter streams 84 MB of Dreamer latents at
// 6.4-6.8 TB/s (13 us), the persistent one takes 17.6 us for the same bytes.
// EMB_SPAN_MOVER=0 sends everything to the flat mover (the fallback).
constexpr int64_t kSpanGatherMB = 160, kSpanScatterMB = 40;
bool span_mover_enabled() {
  static const bool value = [] {
    const char* e = emb::knob("EMB_SPAN_MOVER");
    return !(e && e[0] == '0');
  }();
  return value;
}
// EMB_GATHER_STORES=plain: sample gathers store with plain instead of
// non-temporal stores.  What `nt` stores cost is paid by the NEXT reader of the
// batch, which finds nothing of it in L2 / Infinity Cache: measured with a kernel
// that reads 84 MB of the batch right behind the gather (rocprofv3 medians over
// five GPUs): 13.0-13.4 us behind plain stores, 16.6-18.3 us behind `nt` stores.
// The gather itself is faster with `nt` while the batch is small (60 MB: 12.5
// against 13.5 us) and slower when it is large (144 MB: 26.7 against 25.3 us;
// profiles/r05_ab_gather_stores.txt).  `plain` is the setting for a learner that
// reads the whole batch right after sampling.
int gather_nt() {      // non-temporal hints of a span gather: bit 0 loads, bit 1 stores
  static const int value = [] {
    const char* e = emb::knob("EMB_GATHER_STORES");
    return e && e[0] == 'p' ? 1 : 3;
  }();
  return value;
}
// Compute units of the current device (MI355X: 256), asked once: the persistent
// span mover sizes its grid by it.
int compute_units() {
  static const int value = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    (void)hipGetLastError();
    return n;
  }();
  return value;
}

int pick_unit(const KeyDesc& key) {
  const uint64_t mix = reinterpret_cast<uint64_t>(key.pool) |
                       reinterpret_cast<uint64_t>(key.batch) |
                       static_cast<uint64_t>(key.rowbytes);
  if (mix % 16 == 0) return key.rowbytes >= 2048 ? 0 : 16;
  if (mix % 8 == 0) return 8;
  if (mix % 4 == 0) return 4;
  if (mix % 2 == 0) return 2;
  return 1;
}

// Words of kernel-argument space the plan's tables need, or -1 if they cannot
// go inline.
int inline_words_needed(const MovePlan& plan) {
  int64_t words = 0;
  if (plan.spans_host) words = 3ll * plan.n_seq;
  else if (plan.rows_host) words = plan.n_rows;
  else return plan.inline_key >= 0 ? -1 : 0;
  if (plan.inline_key >= 0) words += static_cast<int64_t>(plan.n_rows) * (plan.key[plan.inline_key].rowbytes >> 2);
  return words <= kInlineWords ? static_cast<int>(words) : -1;
}

static_assert(sizeof(MoveArgs) <= kMoveArgsBytes, "MoveLaunch::args too small");

}  // namespace

hipError_t launch_marker(hipStream_t stream, hipEvent_t stop) {
  hipExtLaunchKernelGGL(marker_kernel, dim3(1), dim3(64), 0, stream, nullptr, stop, 0);
  return hipGetLastError();
}

hipError_t launch_args_writer(const MoveLaunch& launch, void* device_dst, hipStream_t stream,
                              hipEvent_t stop) {
  const MoveArgs& a = *reinterpret_cast<const MoveArgs*>(launch.args);
  // (One writer: one on every XCD -- the block then is in every L2 when the mover
  // asks for it -- measured -0.15 us on the gather and +3.2 us on this kernel.)
  hipExtLaunchKernelGGL(args_writer_kernel, dim3(1), dim3(256), 0, stream, nullptr, stop, 0, a,
                        static_cast<u32x4*>(device_dst));
  return hipGetLastError();
}

hipError_t launch_move(const MoveLaunch& launch, bool gather, const void* device_args,
                       hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
  if (launch.blocks == 0) return hipSuccess;
  const MoveArgs& a = *reinterpret_cast<const MoveArgs*>(launch.args);
  const MoveArgs* ap = static_cast<const MoveArgs*>(device_args);
  const dim3 grid(launch.blocks), block(launch.threads);
#define EMB_LAUNCH(BYVALUE_, INDIRECT_)                                                              \
  do {                                                                                               \
    if (ap) hipExtLaunchKernelGGL(INDIRECT_, grid, block, 0, stream, start, stop, 0, ap);            \
    else hipExtLaunchKernelGGL(BYVALUE_, grid, block, 0, stream, start, stop, 0, a);                 \
  } while (0)
  if (launch.span) {
    if (!gather) EMB_LAUNCH((span_move_kernel<false, 3>), (span_move_kernel_indirect<false, 3>));
    else if (launch.nt == 1) EMB_LAUNCH((span_move_kernel<true, 1>), (span_move_kernel_indirect<true, 1>));
    else EMB_LAUNCH((span_move_kernel<true, 3>), (span_move_kernel_indirect<true, 3>));
  } else if (launch.stage_tables && !ap) {
    if (gather) hipExtLaunchKernelGGL((flat_move_kernel_staged<true>), grid, block, 0, stream, start, stop, 0, a);
    else hipExtLaunchKernelGGL((flat_move_kernel_staged<false>), grid, block, 0, stream, start, stop, 0, a);
  } else {
    if (gather) EMB_LAUNCH((flat_move_kernel<true>), (flat_move_kernel_indirect<true>));
    else EMB_LAUNCH((flat_move_kernel<false>), (flat_move_kernel_indirect<false>));
  }
#undef EMB_LAUNCH
  return hipGetLastError();
}

// The kernel launch_move picks for this launch, spelled as the profiler prints
// it (without namespaces and parameter list).
const char* move_kernel_name(const MoveLaunch& launch, bool gather, bool indirect) {
  static thread_local char name[96];
  if (launch.span)
    std::snprintf(name, sizeof(name), "span_move_kernel%s<%s, %d>", indirect ? "_indirect" : "",
                  gather ? "true" : "false", gather ? launch.nt : 3);
  else
    std::snprintf(name, sizeof(name), "flat_move_kernel%s<%s>",
                  indirect ? "_indirect" : launch.stage_tables ? "_staged" : "", gather ? "true" : "false");
  return name;
}

hipError_t prepare_move(const MovePlan& plan, MoveLaunch* out, bool gather) {
  out->blocks = 0;
  const int inline_need = inline_words_needed(plan);
  const bool use_inline = inline_need > 0 && (plan.spans_host || plan.rows_host);
  if (plan.n_keys < 1 || plan.n_keys > kMaxKeys || plan.n_rows < 0 || (!plan.rows && !use_inline))
    return hipErrorInvalidValue;
  if (plan.n_rows == 0) return hipSuccess;
  // Span tables (sample, windowing, write-back) with at least one wide key go
  // to the persistent span mover; everything else to the flat mover.
  bool span_path = false;
  if (use_inline && plan.spans_host && span_mover_enabled() && plan.seq_len >= 1) {
    int64_t wide_bytes = 0;
    int wide_keys = 0;
    for (int k = 0; k < plan.n_keys; ++k)
      if (!((plan.mask_bits >> k) & 1u) && k != plan.inline_key && pick_unit(plan.key[k]) == 0) {
        const int64_t len = plan.key_len[k] > 0 && plan.key_len[k] < plan.seq_len ? plan.key_len[k] : plan.seq_len;
        wide_bytes += plan.key[k].rowbytes * (static_cast<int64_t>(plan.n_rows) / plan.seq_len) * len;
        ++wide_keys;
      }
    // With host-resident kernel arguments the big movers read their plan from a
    // ring in fine-grained (uncached) device memory: the span mover touches it
    // once per workgroup (the staged head), ~1000 workgroups; the flat mover's
    // ~10 000 short-lived workgroups each fetch their tables and spans from it
    // (staged through LDS since round 6: an 85 MB write-back 20.3 -> 17.1 us,
    // still behind the span mover's 15.2 us; profiles/r06_scatter_lab.txt) --
    // there the span mover takes every size.
    const int64_t limit_mb = gather ? kSpanGatherMB : kSpanScatterMB;
    span_path = wide_bytes > 0 && wide_keys <= kSpanKeys &&
                (plan.args_in_host_memory || wide_bytes <= limit_mb * 1000000);
  }
  const int unroll = span_path ? kSpanUnroll : kFlatUnroll;
  const int threads = span_path ? kSpanThreads : kFlatThreads;
  out->span = span_path;
  out->stage_tables = plan.args_in_host_memory;
  out->nt = gather && span_path ? gather_nt() : 3;
  MoveArgs& a = *reinterpret_cast<MoveArgs*>(out->args);
  SpanHead& h = a.head;
  MoveTables& t = a.t;
  std::memset(&h, 0, sizeof(h));
  for (int j = 0; j < kSpanKeys; ++j) h.tile0[j] = 0xFFFFFFFFu;
  t.group = plan.group > 0 ? plan.group : 0;
  t.group_stride = plan.group_stride;
  h.group = t.group;
  h.group_stride = t.group_stride;
  // Grouped batch sides: gathers and plain write-backs (not the masked insert,
  // not inline step ids), 16-byte aligned groups.
  if (t.group && (plan.group_stride % 16 != 0 || plan.mask_bits || plan.inline_key >= 0))
    return hipErrorInvalidValue;
  t.n_keys = plan.n_keys;
  t.n_rows = plan.n_rows;
  t.seq_len = plan.seq_len < 1 ? 1 : plan.seq_len;
  // Context-only keys (gather): key k moves the first key_len[k] steps of every
  // sequence into a (n_seq, key_len[k], rowbytes) array.
  bool heads = false;
  for (int k = 0; k < plan.n_keys; ++k) {
    if (plan.key_len[k] < 0 || plan.key_len[k] > t.seq_len) return hipErrorInvalidValue;
    heads = heads || (plan.key_len[k] > 0 && plan.key_len[k] < t.seq_len);
  }
  if (heads && (!gather || plan.n_rows % t.seq_len != 0 || plan.mask_bits || plan.inline_key >= 0))
    return hipErrorInvalidValue;
  const int64_t n_seq = plan.n_rows / t.seq_len;
  t.key_is_first = plan.key_is_first;
  t.key_is_last = plan.key_is_last;
  t.is_first_pool = plan.is_first_pool;
  if (!t.is_first_pool && plan.key_is_first >= 0) t.is_first_pool = plan.key[plan.key_is_first].pool;
  t.rows = plan.rows;
  t.rows_mode = 0;
  t.inline_key = -1;
  t.inline_key_word0 = 0;
  if (use_inline) {
    int words;
    if (plan.spans_host) {
      t.rows_mode = 2;
      words = 3 * plan.n_seq;
      std::memcpy(a.inline_words, plan.spans_host, sizeof(uint32_t) * words);
    } else {
      t.rows_mode = 1;
      words = plan.n_rows;
      std::memcpy(a.inline_words, plan.rows_host, sizeof(uint32_t) * words);
    }
    if (plan.inline_key >= 0) {
      t.inline_key = plan.inline_key;
      t.inline_key_word0 = words;
      std::memcpy(a.inline_words + words, plan.inline_bytes,
                  static_cast<size_t>(plan.n_rows) * plan.key[plan.inline_key].rowbytes);
    }
  } else if (plan.inline_key >= 0) {
    return hipErrorInvalidValue;
  }
  t.mask_bits = plan.mask_bits;
  t.mask_flags = plan.mask_flags;
  if (plan.mask_bits && !plan.mask_flags) return hipErrorInvalidValue;
  int64_t blocks = 0;
  for (int k = 0; k < plan.n_keys; ++k) {
    t.key[k] = plan.key[k];
    t.key_len[k] = heads && plan.key_len[k] > 0 ? plan.key_len[k] : t.seq_len;
    t.key_rows[k] = heads ? static_cast<int32_t>(n_seq * t.key_len[k]) : plan.n_rows;
    t.mask_dtype[k] = plan.mask_dtype[k];
    t.mask_out[k] = plan.mask_out[k];
    const bool masked = (plan.mask_bits >> k) & 1u;
    if (masked) {
      const int es = dtype_size(plan.mask_dtype[k]);
      if (es == 0 || plan.key[k].rowbytes % es || k == t.inline_key) return hipErrorInvalidValue;
      t.unit[k] = es;
    } else
    t.unit[k] = (k == t.inline_key) ? 4 : pick_unit(plan.key[k]);
    t.first_block[k] = static_cast<int32_t>(blocks);
    if (t.unit[k] == 0 && span_path) {
      // tiles of threads * unroll units per sequence; no virtual blocks
      const int64_t per_seq = static_cast<int64_t>(t.key_len[k]) * (plan.key[k].rowbytes >> 4);
      const int64_t tps = (per_seq + threads * unroll - 1) / (threads * unroll);
      const int64_t first = h.ntiles;
      if (per_seq > UINT32_MAX / 2 || first + tps * plan.n_seq > UINT32_MAX / 2) return hipErrorInvalidValue;
      h.key[h.n_wide] = plan.key[k];
      h.tiles_per_seq[h.n_wide] = static_cast<uint32_t>(tps);
      h.units_per_seq[h.n_wide] = static_cast<uint32_t>(per_seq);
      h.tile0[h.n_wide] = static_cast<uint32_t>(first);
      h.ntiles = static_cast<uint32_t>(first + tps * plan.n_seq);
      ++h.n_wide;
    } else if (t.unit[k] == 0) {
      const int64_t units = static_cast<int64_t>(t.key_rows[k]) * (plan.key[k].rowbytes >> 4);
      if (units > UINT32_MAX / 2) return hipErrorInvalidValue;
      blocks += (units + threads * unroll - 1) / (threads * unroll);
    } else {
      const int64_t units = static_cast<int64_t>(t.key_rows[k]) * (plan.key[k].rowbytes / t.unit[k]);
      blocks += (units + threads - 1) / threads;
    }
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
  }
  t.first_block[plan.n_keys] = static_cast<int32_t>(blocks);
  out->blocks = static_cast<uint32_t>(blocks);
  if (span_path) {
    // As many workers as the chip takes at once (trimming the count so that
    // every worker walks the same number of tiles was slower with this shape:
    // B=16 10.8 against 10.1 us).
    const int cus = plan.cu_limit > 0 ? std::min(plan.cu_limit, compute_units()) : compute_units();
    const int64_t workers = std::min<int64_t>(h.ntiles, int64_t(cus) * kSpanPerCU);
    h.wide_workers = static_cast<int32_t>(workers);
    h.seq_len = t.seq_len;
    if (blocks + h.wide_workers > INT32_MAX) return hipErrorInvalidValue;
    out->blocks = static_cast<uint32_t>(blocks + h.wide_workers);
  }
  out->threads = static_cast<uint32_t>(threads);
  return hipSuccess;
}

size_t move_args_bytes() { return sizeof(MoveArgs); }

hipError_t launch_gather(const MovePlan& plan, hipStream_t stream, hipEvent_t start,
                         hipEvent_t stop) {
  MoveLaunch launch;
  const hipError_t e = prepare_move(plan, &launch, true);
  return e != hipSuccess ? e : launch_move(launch, true, nullptr, stream, start, stop);
}

bool plan_fits_inline(const MovePlan& plan) { return inline_words_needed(plan) > 0; }

hipError_t launch_scatter(const MovePlan& plan, hipStream_t stream) {
  MoveLaunch launch;
  const hipError_t e = prepare_move(plan, &launch, false);
  return e != hipSuccess ? e : launch_move(launch, false, nullptr, stream, nullptr, nullptr);
}

}  // namespace emb
