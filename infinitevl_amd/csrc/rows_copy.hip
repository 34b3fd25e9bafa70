// Row fork: copies row `src_row` of every tensor of a table to a set of rows of the partner tensors, in ONE launch
// (ivl_rows_copy_fwd).  A stream's whole history is one row each of ~130 tensors of very different sizes (2 MB ring rows,
// 1 MiB recurrent states, 16-32 KB conv states, 8-byte counters): the rows are cut into pieces of RC_CHUNK bytes, the
// pieces of all entries form one flat work list (the table's sixth column is each entry's first piece), and the workgroups
// take equal contiguous shares of that list -- the load on the chip does not depend on the mix of entries.
// Every source byte is loaded once and stored to every destination.  No LDS, plain vector stores.
#include "ivl_common.h"

namespace ivl {

constexpr int RC_COLS = 6;          // src_base, dst_base, src_row_stride_bytes, dst_row_stride_bytes, row_bytes, first_piece
constexpr int RC_CHUNK = 16384;     // bytes of a row per work item (a multiple of 16)
constexpr int RC_THREADS = 256;
constexpr int RC_VECS = RC_CHUNK / 16 / RC_THREADS;   // 16-byte pieces per thread and work item: all loaded before the first store
constexpr int RC_MAX_GRID = 8192;      // more workgroups than are resident at once: they start staggered, loads overlap stores

// the table holds addresses as integers: tell the compiler they are global memory (global_load / global_store, not flat)
typedef __attribute__((address_space(1))) u32x4 rc_gvec;
typedef __attribute__((address_space(1))) unsigned char rc_gbyte;

__device__ __forceinline__ long long rc_pieces(long long row_bytes) { return (row_bytes + RC_CHUNK - 1) / RC_CHUNK; }

// (leading scalars first: they arrive preloaded in SGPRs)
__global__ __launch_bounds__(RC_THREADS) void rows_copy_kernel(int n_entries, int src_row, unsigned long long dst_mask,
                                                               const long long* __restrict__ table) {
  // Everything read from the table is uniform over the workgroup and indexed by uniform values: scalar loads through the
  // scalar cache, which the whole table fits (vector loads of it from every wave crowd the few L2 channels it lives in).
  const int tid = threadIdx.x;
  const long long* last = table + (long long)(n_entries - 1) * RC_COLS;
  const long long total = last[5] + rc_pieces(last[4]);
  const long long per = (total + gridDim.x - 1) / gridDim.x;
  long long item = (long long)blockIdx.x * per;
  if (item >= total) return;
  const long long item_end = item + per < total ? item + per : total;

  // the entry of the first item: the last one whose first piece is at or before it (entry 0 starts at piece 0)
  int e = 0;
  for (int hi_e = n_entries; hi_e - e > 1;) {
    const int mid = (e + hi_e) >> 1;
    if (table[(long long)mid * RC_COLS + 5] <= item) e = mid;
    else hi_e = mid;
  }
  const long long* ent = table + (long long)e * RC_COLS;
  long long piece = item - ent[5];

  for (; item < item_end; ++item, ++piece) {
    long long row_bytes = ent[4];
    if (piece >= rc_pieces(row_bytes)) {          // (every entry has at least one piece: one step is enough)
      ++e;
      ent += RC_COLS;
      piece = 0;
      row_bytes = ent[4];
    }
    const long long src_base = ent[0], dst_base = ent[1];
    const long long dst_stride = ent[3];
    const long long s = src_base + (long long)src_row * ent[2];
    // a row is never copied onto itself
    const unsigned long long mask = src_base == dst_base ? dst_mask & ~(1ull << src_row) : dst_mask;
    const long long lo = piece * RC_CHUNK;
    const long long hi = lo + RC_CHUNK < row_bytes ? lo + RC_CHUNK : row_bytes;

    // 16-byte pieces need the source and every destination at the same offset inside a 16-byte line
    unsigned int rel = 0;
    for (unsigned long long m = mask; m; m &= m - 1) {
      const int r = __builtin_ctzll(m);
      rel |= (unsigned int)((unsigned long long)(dst_base + (long long)r * dst_stride) - (unsigned long long)s);
    }
    if ((rel & 15u) == 0) {
      long long a = lo + (long long)((0 - (unsigned long long)(s + lo)) & 15u);      // head [lo, a): bytes
      if (a > hi) a = hi;
      const long long nvec = (hi - a) >> 4;                                            // body [a, b): 16-byte pieces
      const long long b = a + (nvec << 4);                                             // tail [b, hi): bytes
      u32x4 v[RC_VECS];
#pragma unroll
      for (int k = 0; k < RC_VECS; ++k) {
        const long long idx = tid + k * RC_THREADS;
        if (idx < nvec) v[k] = *(const rc_gvec*)(s + a + idx * 16);
      }
      long long off = -1;
      if (tid < a - lo) off = lo + tid;
      else if (tid >= 16 && tid - 16 < hi - b) off = b + (tid - 16);
      unsigned char edge = 0;
      if (off >= 0) edge = *(const rc_gbyte*)(s + off);
      for (unsigned long long m = mask; m; m &= m - 1) {
        const long long d = dst_base + (long long)__builtin_ctzll(m) * dst_stride;
#pragma unroll
        for (int k = 0; k < RC_VECS; ++k) {
          const long long idx = tid + k * RC_THREADS;
          if (idx < nvec) *(rc_gvec*)(d + a + idx * 16) = v[k];
        }
        if (off >= 0) *(rc_gbyte*)(d + off) = edge;
      }
    } else {
      for (long long off = lo + tid; off < hi; off += RC_THREADS) {
        const unsigned char c = *(const rc_gbyte*)(s + off);
        for (unsigned long long m = mask; m; m &= m - 1)
          *(rc_gbyte*)(dst_base + (long long)__builtin_ctzll(m) * dst_stride + off) = c;
      }
    }
  }
}

// Row gather (ivl_rows_gather_fwd): row row0 + d of every entry <- the OLD row row0 + parent[d], for all d < n_rows at once, in
// place, the map read from the device.  The work list, the pieces and the table search are those of rows_copy_kernel.  No shadow
// copy and no barrier: for its own 16-byte lanes (and edge bytes) of a piece a thread first loads that lane from every row that
// some d != parent[d] names, and only then stores to every such d -- a thread only ever overwrites bytes it has itself already
// loaded, and no other thread touches the same offset of any row, so cycles, swaps and fan-out need no ordering between threads.
// NR: the register sets (rows of the group); HALVES: a piece is walked in HALVES parts, so NR * RC_VECS / HALVES 16-byte
// registers hold a part of every row (NR = 4: 4 x 4, NR = 8: 8 x 2 -- 64 VGPRs either way).  `parent` is uniform: the sets are
// selected by uniform branches over unrolled indices, never by a register index.
template <int NR, int HALVES>
__global__ __launch_bounds__(RC_THREADS) void rows_gather_kernel(int n_entries, int row0, int n_rows,
                                                                 const int* __restrict__ parent,
                                                                 const long long* __restrict__ table) {
  constexpr int SUB = RC_CHUNK / HALVES;
  constexpr int VECS = RC_VECS / HALVES;
  const int tid = threadIdx.x;
  // the map: par[d] in [0, n_rows), anything else counts as d; moved = the rows that change, need = the rows they read
  int par[NR];
  unsigned moved = 0u, need = 0u;
#pragma unroll
  for (int d = 0; d < NR; ++d) {
    par[d] = d;
    if (d < n_rows) {
      const int p = parent[d];
      if (p >= 0 && p < n_rows && p != d) { par[d] = p; moved |= 1u << d; need |= 1u << p; }
    }
  }
  if (moved == 0u) return;                           // the identity: no byte is loaded or stored

  const long long* last = table + (long long)(n_entries - 1) * RC_COLS;
  const long long total = last[5] + rc_pieces(last[4]);
  const long long per = (total + gridDim.x - 1) / gridDim.x;
  long long item = (long long)blockIdx.x * per;
  if (item >= total) return;
  const long long item_end = item + per < total ? item + per : total;
  int e = 0;
  for (int hi_e = n_entries; hi_e - e > 1;) {
    const int mid = (e + hi_e) >> 1;
    if (table[(long long)mid * RC_COLS + 5] <= item) e = mid;
    else hi_e = mid;
  }
  const long long* ent = table + (long long)e * RC_COLS;
  long long piece = item - ent[5];

  for (; item < item_end; ++item, ++piece) {
    long long row_bytes = ent[4];
    if (piece >= rc_pieces(row_bytes)) {
      ++e;
      ent += RC_COLS;
      piece = 0;
      row_bytes = ent[4];
    }
    const long long stride = ent[3];
    const long long g0 = ent[1] + (long long)row0 * stride;      // row row0 of the entry (src_base == dst_base)
    for (int h = 0; h < HALVES; ++h) {
      const long long lo = piece * RC_CHUNK + (long long)h * SUB;
      if (lo >= row_bytes) break;
      const long long hi = lo + SUB < row_bytes ? lo + SUB : row_bytes;
      if ((stride & 15) == 0) {                      // every row of the group at the same offset inside a 16-byte line
        long long a = lo + (long long)((0 - (unsigned long long)(g0 + lo)) & 15u);     // head [lo, a): bytes
        if (a > hi) a = hi;
        const long long nvec = (hi - a) >> 4;                                           // body [a, b): 16-byte pieces
        const long long b = a + (nvec << 4);                                            // tail [b, hi): bytes
        long long off = -1;
        if (tid < a - lo) off = lo + tid;
        else if (tid >= 16 && tid - 16 < hi - b) off = b + (tid - 16);
        u32x4 v[NR][VECS];
        unsigned char edge[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          edge[r] = 0;
          if (need >> r & 1u) {
            const long long s = g0 + (long long)r * stride;
#pragma unroll
            for (int k = 0; k < VECS; ++k) {
              const long long idx = tid + k * RC_THREADS;
              if (idx < nvec) v[r][k] = *(const rc_gvec*)(s + a + idx * 16);
            }
            if (off >= 0) edge[r] = *(const rc_gbyte*)(s + off);
          }
        }
#pragma unroll
        for (int d = 0; d < NR; ++d) {
          if (moved >> d & 1u) {
            const long long t = g0 + (long long)d * stride;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
              if (par[d] == r) {
#pragma unroll
                for (int k = 0; k < VECS; ++k) {
                  const long long idx = tid + k * RC_THREADS;
                  if (idx < nvec) *(rc_gvec*)(t + a + idx * 16) = v[r][k];
                }
                if (off >= 0) *(rc_gbyte*)(t + off) = edge[r];
              }
            }
          }
        }
      } else {
        for (long long off = lo + tid; off < hi; off += RC_THREADS) {
          unsigned char c[NR];
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            c[r] = 0;
            if (need >> r & 1u) c[r] = *(const rc_gbyte*)(g0 + (long long)r * stride + off);
          }
#pragma unroll
          for (int d = 0; d < NR; ++d) {
            if (moved >> d & 1u) {
#pragma unroll
              for (int r = 0; r < NR; ++r)
                if (par[d] == r) *(rc_gbyte*)(g0 + (long long)d * stride + off) = c[r];
            }
          }
        }
      }
    }
  }
}

}  // namespace ivl

using namespace ivl;

extern "C" int ivl_rows_gather_fwd(const int64_t* table, int n_entries, int64_t max_row_bytes, int row0, int n_rows,
                                   const int32_t* parent, void* stream) {
  IVL_REQUIRE(table && parent, IVL_ERR_INVALID_ARG, "ivl_rows_gather_fwd: NULL %s", table ? "parent" : "table");
  IVL_REQUIRE(n_entries >= 1, IVL_ERR_INVALID_ARG, "ivl_rows_gather_fwd: n_entries=%d must be >= 1", n_entries);
  IVL_REQUIRE(max_row_bytes >= 1, IVL_ERR_INVALID_ARG, "ivl_rows_gather_fwd: max_row_bytes=%lld must be >= 1", (long long)max_row_bytes);
  IVL_REQUIRE(row0 >= 0, IVL_ERR_INVALID_ARG, "ivl_rows_gather_fwd: row0=%d must be >= 0", row0);
  IVL_REQUIRE(n_rows >= 1 && n_rows <= 8, IVL_ERR_INVALID_ARG, "ivl_rows_gather_fwd: n_rows=%d outside 1..8", n_rows);
  IVL_REQUIRE(row0 + n_rows <= 63, IVL_ERR_UNSUPPORTED, "ivl_rows_gather_fwd: rows >= 63 are unsupported (row0=%d, n_rows=%d)", row0,
              n_rows);
  long long grid = (long long)n_entries * ((max_row_bytes + RC_CHUNK - 1) / RC_CHUNK);
  if (grid > RC_MAX_GRID || grid < 1) grid = RC_MAX_GRID;
  if (n_rows <= 4)
    hipLaunchKernelGGL((rows_gather_kernel<4, 1>), dim3((int)grid), dim3(RC_THREADS), 0, (hipStream_t)stream, n_entries, row0, n_rows,
                       (const int*)parent, (const long long*)table);
  else
    hipLaunchKernelGGL((rows_gather_kernel<8, 2>), dim3((int)grid), dim3(RC_THREADS), 0, (hipStream_t)stream, n_entries, row0, n_rows,
                       (const int*)parent, (const long long*)table);
  return check_launch("ivl_rows_gather_fwd");
}

extern "C" int ivl_rows_copy_fwd(const int64_t* table, int n_entries, int64_t max_row_bytes, int src_row, int64_t dst_mask,
                                 void* stream) {
  IVL_REQUIRE(table, IVL_ERR_INVALID_ARG, "ivl_rows_copy_fwd: NULL table");
  IVL_REQUIRE(n_entries >= 1, IVL_ERR_INVALID_ARG, "ivl_rows_copy_fwd: n_entries=%d must be >= 1", n_entries);
  IVL_REQUIRE(max_row_bytes >= 1, IVL_ERR_INVALID_ARG, "ivl_rows_copy_fwd: max_row_bytes=%lld must be >= 1", (long long)max_row_bytes);
  IVL_REQUIRE(src_row >= 0, IVL_ERR_INVALID_ARG, "ivl_rows_copy_fwd: src_row=%d must be >= 0", src_row);
  IVL_REQUIRE(dst_mask != 0, IVL_ERR_INVALID_ARG, "ivl_rows_copy_fwd: dst_mask is empty");
  IVL_REQUIRE(src_row < 63 && dst_mask > 0, IVL_ERR_UNSUPPORTED, "ivl_rows_copy_fwd: rows >= 63 are unsupported (src_row=%d, dst_mask=0x%llx)",
              src_row, (unsigned long long)dst_mask);
  // an upper bound of the work list (the table lives on the device); the kernel reads the true length from the table
  long long grid = (long long)n_entries * ((max_row_bytes + RC_CHUNK - 1) / RC_CHUNK);
  if (grid > RC_MAX_GRID || grid < 1) grid = RC_MAX_GRID;
  hipLaunchKernelGGL(rows_copy_kernel, dim3((int)grid), dim3(RC_THREADS), 0, (hipStream_t)stream, n_entries, src_row,
                     (unsigned long long)dst_mask, (const long long*)table);
  return check_launch("ivl_rows_copy_fwd");
}
