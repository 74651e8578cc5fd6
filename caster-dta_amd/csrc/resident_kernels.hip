// resident_kernels.hip -- collate a batch from a resident set of unique graphs (include/caster_gvp_resident.h; opt-in).
//
// The reference keeps a dataset's unique graphs once and lets the pairs index into them (dataset/dual_dataset.py:
// 123-125), yet its collator concatenates the same graphs on the host and ships them again every step (:526-547).
// Here the concatenation of ALL unique graphs of one side lives on the device and
//
//   collate_kernel   one launch per side and batch: every item (a feature tensor, a row of edge_index, `batch`) is cut
//                    into tiles of 256 destination vectors of 16 bytes, the tiles of all items form one flat list that
//                    the workgroups walk with a grid stride, one vector per lane and tile
//
// The unit of work is a 16-byte ALIGNED 16 bytes of an item's DESTINATION, not a graph: row sizes are 68, 36, 8, 128,
// 12 and 164 bytes, so a graph's segment starts anywhere on a 4-byte grid, on both sides independently, and a one-node
// graph is an 8-byte segment.  A lane finds the position its first word belongs to by bisecting the batch's offset
// table (log2 B loads that hit the L2), walks on to the next position where its four words cross a boundary, gathers
// the words from the resident tensor (one 16-byte load where the four source words are adjacent and aligned, 4-byte
// loads otherwise: the source misaligns against the destination in three cases out of four) and stores 16 bytes once.
// Only the first and the last vector of an ITEM can be partial; they store their words one by one.  So every byte of a
// destination is written once, by one lane, nothing outside [dst, dst + bytes) is written, and nothing but the source
// words of selected graphs is read.  No LDS, no atomics, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/caster_gvp_resident.h"
#include "gvp_host.h"

namespace {

constexpr int THREADS = 256;          // vectors of a tile: 4 KB of destination
constexpr int DEFAULT_BLOCKS = 2048;  // 8 workgroups a CU; more tiles than that are walked with the grid stride

struct Item {
  char* dst;
  const char* src;
  int64_t bytes;   // rows * row_bytes
  int64_t tile0;   // first tile of the item in the flat list
  int32_t row_bytes, kind;
  int32_t lead;    // dst & 15: vector v covers the item's bytes [16 v - lead, 16 v - lead + 16)
};

struct Params {
  Item it[CGVP_COLLATE_MAX_ITEMS];
  const int64_t *sel, *dst_node_off, *dst_edge_off, *src_node_off, *src_edge_off;
  int64_t positions, tiles;
  int32_t items;
};

// The position a row of the batch lies in: `b`, the first row behind it, and what takes a row of the batch to its row
// in the resident tensor.
struct Seg {
  int64_t b, end, delta;
};

struct Tables {
  const int64_t *dst_off, *src_off, *sel;
  int64_t positions;

  // largest b with dst_off[b] <= r (r < dst_off[positions]): dst_off[b] <= r < dst_off[b + 1], position b has rows
  __device__ Seg find(int64_t r) const {
    int64_t lo = 0, hi = positions;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (dst_off[mid] <= r) lo = mid; else hi = mid;
    }
    return Seg{lo, dst_off[lo + 1], src_off[sel[lo]] - dst_off[lo]};
  }
  // `s` for a later row r (positions without rows are stepped over)
  __device__ void advance(Seg& s, int64_t r) const {
    if (r < s.end) return;
    do { ++s.b; s.end = dst_off[s.b + 1]; } while (r >= s.end);
    s.delta = src_off[sel[s.b]] - dst_off[s.b];
  }
};

// Opaque rows of row_bytes (a multiple of 4): vector `v` of the item.
__device__ inline void copy_vector(const Item& it, const Tables& t, int64_t v) {
  const int64_t o = 16 * v - it.lead;                           // the item's byte the vector starts at (< 0: head)
  const int w0 = o < 0 ? (int)(-o >> 2) : 0;                    // words w0 .. w1-1 of the vector lie in the item
  const int64_t left = it.bytes - o;
  const int w1 = left >= 16 ? 4 : (int)(left >> 2);
  const int64_t first = o + 4 * w0;
  const int32_t rb = it.row_bytes;
  int64_t r = (first >> 32) ? first / rb : (int64_t)((uint32_t)first / (uint32_t)rb);
  int32_t rem = (int32_t)(first - r * rb);
  Seg s = t.find(r);
  const uint32_t* p[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    p[w] = nullptr;
    if (w >= w0 && w < w1) {
      t.advance(s, r);
      p[w] = reinterpret_cast<const uint32_t*>(it.src + (r + s.delta) * rb + rem);
      rem += 4;
      if (rem >= rb) { rem = 0; ++r; }
    }
  }
  if (w0 == 0 && w1 == 4) {
    uint4 val;
    if (p[1] == p[0] + 1 && p[2] == p[0] + 2 && p[3] == p[0] + 3 && !((uintptr_t)p[0] & 15)) {
      val = *reinterpret_cast<const uint4*>(p[0]);
    } else {
      val.x = *p[0]; val.y = *p[1]; val.z = *p[2]; val.w = *p[3];
    }
    *reinterpret_cast<uint4*>(it.dst + o) = val;
    return;
  }
  uint32_t* d = reinterpret_cast<uint32_t*>(it.dst + o);        // an end of the item: o itself may lie in front of dst
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (w >= w0 && w < w1) d[w] = *p[w];
}

// int64 rows whose value depends on the position: an endpoint row of edge_index (+ the position's first node) or `batch`.
__device__ inline void index_vector(const Item& it, const Tables& t, const int64_t* dst_node_off, int64_t v) {
  const int64_t o = 16 * v - it.lead;                           // lead is 0 or 8
  const int u0 = o < 0 ? 1 : 0;
  const int u1 = it.bytes - o >= 16 ? 2 : 1;
  const bool ends = it.kind == CGVP_COLLATE_ENDPOINTS;
  int64_t r = (o >> 3) + u0;
  Seg s = t.find(r);
  const int64_t* src = reinterpret_cast<const int64_t*>(it.src);
  int64_t* d = reinterpret_cast<int64_t*>(it.dst + o);
  if (u0 == 0 && u1 == 2) {
    const Seg s0 = s;
    t.advance(s, r + 1);
    longlong2 val;
    if (ends) {
      const int64_t* a = src + (r + s0.delta);
      const int64_t* b = src + (r + 1 + s.delta);
      if (b == a + 1 && !((uintptr_t)a & 15)) {
        val = *reinterpret_cast<const longlong2*>(a);
      } else {
        val.x = *a; val.y = *b;
      }
      val.x += dst_node_off[s0.b];
      val.y += dst_node_off[s.b];
    } else {
      val.x = s0.b; val.y = s.b;
    }
    *reinterpret_cast<longlong2*>(d) = val;
    return;
  }
  d[u0] = ends ? src[r + s.delta] + dst_node_off[s.b] : s.b;
}

__global__ __launch_bounds__(THREADS) void collate_kernel(Params p) {
  for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    int i = 0;
    while (i + 1 < p.items && tile >= p.it[i + 1].tile0) ++i;   // uniform: the item of this tile
    const Item& it = p.it[i];
    const int64_t v = (tile - it.tile0) * THREADS + threadIdx.x;
    if (16 * v - it.lead >= it.bytes) continue;                 // behind the item's last vector
    const bool edges = it.kind == CGVP_COLLATE_EDGE_ROWS || it.kind == CGVP_COLLATE_ENDPOINTS;
    const Tables t{edges ? p.dst_edge_off : p.dst_node_off, edges ? p.src_edge_off : p.src_node_off, p.sel, p.positions};
    if (it.kind == CGVP_COLLATE_ENDPOINTS || it.kind == CGVP_COLLATE_BATCH) index_vector(it, t, p.dst_node_off, v);
    else copy_vector(it, t, v);
  }
}

}  // namespace

extern "C" {

int cgvp_resident_version(void) { return CGVP_RESIDENT_VERSION; }

int cgvp_collate_graphs(const cgvp_collate_item* items, int32_t num_items, const int64_t* sel,
                        const int64_t* dst_node_off, const int64_t* dst_edge_off, const int64_t* src_node_off,
                        const int64_t* src_edge_off, int64_t num_positions, int64_t num_nodes, int64_t num_edges,
                        int32_t max_blocks, void* stream) {
  constexpr int64_t MAX_ROWS = int64_t(1) << 40;
  if (num_items < 0 || num_items > CGVP_COLLATE_MAX_ITEMS || (num_items > 0 && !items)) return CGVP_ERR_BAD_ARG;
  if (bad_ptr(sel, 8) || bad_ptr(dst_node_off, 8) || bad_ptr(dst_edge_off, 8) || bad_ptr(src_node_off, 8) ||
      bad_ptr(src_edge_off, 8))
    return CGVP_ERR_BAD_ARG;
  if (num_positions < 0 || num_positions >= (int64_t(1) << 30) || num_nodes < 0 || num_nodes >= MAX_ROWS ||
      num_edges < 0 || num_edges >= MAX_ROWS || max_blocks < 0)
    return CGVP_ERR_BAD_ARG;
  Params p;
  p.sel = sel; p.dst_node_off = dst_node_off; p.dst_edge_off = dst_edge_off;
  p.src_node_off = src_node_off; p.src_edge_off = src_edge_off;
  p.positions = num_positions;
  p.items = 0;
  int64_t tiles = 0;
  for (int i = 0; i < num_items; ++i) {
    const cgvp_collate_item& in = items[i];
    if (in.kind < CGVP_COLLATE_NODE_ROWS || in.kind > CGVP_COLLATE_BATCH) return CGVP_ERR_BAD_ARG;
    const bool index = in.kind == CGVP_COLLATE_ENDPOINTS || in.kind == CGVP_COLLATE_BATCH;
    if (in.row_bytes < 4 || in.row_bytes > (1 << 20) || (in.row_bytes & 3) || (index && in.row_bytes != 8)) return CGVP_ERR_BAD_ARG;
    const uintptr_t align = index ? 7 : 3;
    if (((uintptr_t)in.dst & align) || (in.kind != CGVP_COLLATE_BATCH && ((uintptr_t)in.src & align))) return CGVP_ERR_BAD_ARG;
    const int64_t rows = (in.kind == CGVP_COLLATE_NODE_ROWS || in.kind == CGVP_COLLATE_BATCH) ? num_nodes : num_edges;
    if (rows > 0 && (!in.dst || (in.kind != CGVP_COLLATE_BATCH && !in.src))) return CGVP_ERR_BAD_ARG;
    if (rows == 0) continue;                                    // nothing to write: not an item of the launch
    Item& it = p.it[p.items++];
    it.dst = static_cast<char*>(in.dst);
    it.src = static_cast<const char*>(in.src);
    it.bytes = rows * in.row_bytes;
    it.tile0 = tiles;
    it.row_bytes = in.row_bytes;
    it.kind = in.kind;
    it.lead = (int32_t)((uintptr_t)in.dst & 15);
    const int64_t vectors = (it.lead + it.bytes + 15) / 16;
    tiles += (vectors + THREADS - 1) / THREADS;
  }
  if (num_positions == 0 || tiles == 0) return 0;
  p.tiles = tiles;
  const int64_t cap = max_blocks > 0 ? max_blocks : DEFAULT_BLOCKS;
  const int64_t blocks = tiles < cap ? tiles : cap;
  launch<collate_kernel>(dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, p);
  return launch_status();
}

}  // extern "C"
