/*
 * caster_gvp_resident.h -- collate a batch on the device from a resident set of unique graphs.
 *
 * A CASTER-DTA dataset is a few hundred unique graphs reused across tens of thousands of pairs.  The unique graphs of
 * one side are kept on the device as ONE concatenation per field (node rows, edge rows, edge_index with graph-LOCAL
 * node ids) with two offset tables; cgvp_collate_graphs assembles any batch of them -- any order, repeats allowed -- in
 * ONE launch that only copies, rebases and fills.  The result is bitwise what concatenating the selected graphs on
 * the host and uploading them gives.
 *
 * A header and a version of its own beside the main C ABI (caster_gvp.h and CGVP_ABI_VERSION do not move).  Same
 * library, same conventions: caller-owned DEVICE pointers, nothing allocated or retained, an explicit hipStream_t,
 * asynchronous launches, 0 = launched / >0 = hipError_t / <0 = CGVP_ERR_* from caster_gvp.h, re-entrant, no state.
 * Nothing is read back: the call can be captured into a HIP graph, and overwriting the tables in place replays
 * another batch of the same totals.
 */
#ifndef CASTER_GVP_RESIDENT_H
#define CASTER_GVP_RESIDENT_H

#include <stdint.h>

#include "caster_gvp.h" /* CGVP_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define CGVP_RESIDENT_VERSION 1

int cgvp_resident_version(void);

#define CGVP_COLLATE_MAX_ITEMS 16

/* What one item of a collate launch does.  Position b of the batch holds unique graph g = sel[b]. */
#define CGVP_COLLATE_NODE_ROWS 0 /* dst rows dst_node_off[b] .. = src rows src_node_off[g] .., opaque bytes          */
#define CGVP_COLLATE_EDGE_ROWS 1 /* dst rows dst_edge_off[b] .. = src rows src_edge_off[g] .., opaque bytes          */
#define CGVP_COLLATE_ENDPOINTS 2 /* int64 edge rows: the same copy as EDGE_ROWS, plus dst_node_off[b] (local node
                                    ids become ids of the batch); one row of a [2, E] edge_index per item             */
#define CGVP_COLLATE_BATCH 3     /* int64 node rows: dst row = b for every node of position b; src is not read       */

typedef struct {
  void* dst;         /* [rows of the batch][row_bytes]: num_nodes rows (NODE_ROWS, BATCH) or num_edges (the others)   */
  const void* src;   /* the resident tensor, [rows of all unique graphs][row_bytes]; ignored for BATCH               */
  int32_t row_bytes; /* a multiple of 4; 8 for ENDPOINTS and BATCH                                                   */
  int32_t kind;      /* CGVP_COLLATE_*                                                                               */
} cgvp_collate_item;

/* One launch for all items of one side of a batch.
 *
 * Device tables, int64, 8-byte aligned: sel [num_positions] unique-graph index of every position; dst_node_off /
 * dst_edge_off [num_positions + 1] ascending row offsets of the positions in the batch, [0] == 0 and [num_positions]
 * == num_nodes / num_edges (dst_node_off IS the batch's `ptr`); src_node_off / src_edge_off [unique graphs + 1] row
 * offsets of the unique graphs in the resident tensors.  The caller guarantees
 *   dst_node_off[b+1] - dst_node_off[b] == src_node_off[sel[b]+1] - src_node_off[sel[b]]   (the same for edges)
 * and sel[b] inside the resident set: the kernel cannot check device tables and trusts them.  A graph without nodes
 * or without edges is legal.
 *
 * Rows are only 4-byte aligned and the source and the destination of a segment misalign independently.  Every 16-byte
 * aligned 16 bytes of an item's destination are written by one lane with one 16-byte store (gathered from up to four
 * segments where short graphs meet); the at most two partial vectors at the two ends of an item's destination are
 * written with 4-byte (8-byte for the int64 kinds) stores.  No byte outside [dst, dst + rows * row_bytes) is written
 * and no byte outside the selected graphs' source rows is read.
 *
 * num_nodes / num_edges are the host-known totals of the batch: they size the grid.  max_blocks caps the grid
 * (0 = the default cap); with fewer workgroups than tiles each one walks several tiles.
 *
 * CGVP_ERR_BAD_ARG, before anything is launched: items NULL with num_items > 0, num_items outside
 * 0 .. CGVP_COLLATE_MAX_ITEMS, a NULL table or one that is not 8-byte aligned, num_positions < 0 or >= 2^30, num_nodes
 * or num_edges < 0 or >= 2^40, max_blocks < 0, an unknown kind, a row_bytes < 4, > 2^20 or no multiple of 4 (not 8 for
 * the int64 kinds), a dst (or a src that is read) that is NULL while the item has rows, or not aligned to 4 bytes
 * (8 bytes for the int64 kinds).  With no position or no byte to write nothing is launched and the call returns 0. */
int cgvp_collate_graphs(const cgvp_collate_item* items, int32_t num_items, const int64_t* sel,
                        const int64_t* dst_node_off, const int64_t* dst_edge_off, const int64_t* src_node_off,
                        const int64_t* src_edge_off, int64_t num_positions, int64_t num_nodes, int64_t num_edges,
                        int32_t max_blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CASTER_GVP_RESIDENT_H */
