/*
 * caster_gvp_structure.h -- backbone coordinates -> protein graph on the device.
 *
 * A header of its own beside caster_gvp.h: the entry points below live in the same libcaster_gvp.so, follow the
 * same conventions (caller-owned DEVICE pointers, contiguous row-major tensors, nothing allocated or retained, an
 * explicit hipStream_t, asynchronous launches, 0 = launched / >0 = hipError_t / <0 = CGVP_ERR_* from caster_gvp.h,
 * re-entrant, no state), and carry a version of their own, so the main C ABI does not move when this one grows.
 *
 * Together with cgvp_edge_featurise (caster_gvp.h) they replace the reference's per-protein CPU featuriser:
 * utils/create_protein_features.py:12-198 (nodes), :201-357 (edges) and the COO construction + NaN filter of
 * utils/create_graphs.py:29,44-45.
 *
 * BATCHES.  `ptr` is int64 [num_graphs + 1]: graph b owns the rows ptr[b] .. ptr[b+1] of every per-residue tensor.
 * Nothing crosses a graph: no dihedral, no chain step, no edge.  Offsets are clamped to [0, num_nodes] and a row
 * that no graph owns (malformed ptr) is treated as a graph of one residue; nothing is read or written out of bounds.
 */
#ifndef CASTER_GVP_STRUCTURE_H
#define CASTER_GVP_STRUCTURE_H

#include <stdint.h>

#include "caster_gvp.h" /* CGVP_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

#define CGVP_STRUCTURE_VERSION 1
#define CGVP_KNN_MAX 64 /* largest k of cgvp_knn_graph_select */

int cgvp_structure_version(void);

/* ------------------------------------------------------------ NODE FEATURES
 * utils/create_protein_features.py:27-92 with vectorize_features=True, no ESM-2 columns, no residue positional
 * encoding.  coords [N][4][3] fp32, backbone atoms in N, CA, C, O order (Angstrom); types [N] int64; props
 * [num_types][num_props] fp32, the caller's per-residue-type property table (the reference's 11 amino-acid
 * properties, :99-109; num_props = 0 leaves the columns out and props may be NULL).  A type outside
 * [0, num_types) reads the nearest row.  All geometry is computed in fp64 from the fp32 coordinates, stored fp32.
 *   x_s[n][0:3] = cos(phi, psi, omega), x_s[n][3:6] = sin(phi, psi, omega)                              (:34-66)
 *     dihedrals of the graph's own flattened N, CA, C chain: angle = arccos(clip(n1.n2)) sign(n1.u2); the first
 *     phi and the last psi / omega of a graph are the angle 0 (cos 1, sin 0); a zero-length difference or cross
 *     product normalises to the zero vector (normalize_vecs :360-365)
 *   x_s[n][6:6+num_props] = props[types[n]]                                                              (:97-109)
 *   x_v[n][0] = unit(CA_{n+1} - CA_n), zero on the graph's last residue                                 (:73-77)
 *   x_v[n][1] = -unit(CA_n - CA_{n-1}), zero on the graph's first residue
 *   x_v[n][2] = -bisector sqrt(1/3) - perp sqrt(2/3), bisector = unit(unit(N - CA) + unit(C - CA)),
 *               perp = unit(unit(C - CA) x unit(N - CA))                                                 (:84-92)
 * x_s [N][6 + num_props], x_v [N][3][3].  Optional outputs (NULL to skip): batch [N] int64 = graph of the row,
 * seq [N] int64 = position of the residue inside its graph (the seq_index cgvp_edge_featurise takes).  One launch. */
int cgvp_node_featurise(const float* coords, const int64_t* types, const int64_t* ptr, const float* props,
                        int64_t num_nodes, int64_t num_graphs, int32_t num_types, int32_t num_props, float* x_s,
                        float* x_v, int64_t* batch, int64_t* seq, void* stream);

/* ------------------------------------------------------------ EDGE LIST
 * The edges i -> j the reference keeps (utils/create_protein_features.py:290-331), in the row-major COO order of
 * utils/create_graphs.py:29,44-45: sources non-decreasing, targets increasing within a source.  ca_xyz [N][3] fp32
 * C-alpha positions; squared distances are formed and compared in fp64 on the up-cast coordinates.  With
 * keep_self_loops == 0 the pair (i, i) is never a candidate (:279-282).
 *
 * thresh_type 'dist' (:293-301): cgvp_radius_graph_count writes deg[i] = #{j in graph(i) : |CA_i - CA_j|^2 <=
 * radius^2} (int64 [N]); the caller forms rowstart = exclusive scan of deg and E = its total, then cgvp_graph_fill
 * with tau_d2 = tau_j = NULL writes edge_index. */
int cgvp_radius_graph_count(const float* ca_xyz, const int64_t* ptr, int64_t num_nodes, int64_t num_graphs,
                            double radius, int32_t keep_self_loops, int64_t* deg, void* stream);

/* thresh_type 'num' (:309-327), 1 <= k <= CGVP_KNN_MAX: per source i the k-th smallest key (|CA_i - CA_j|^2, j) over
 * the candidates j of its graph, written as tau_d2[i] (double) / tau_j[i] (int64), and deg[i] = min(k, candidates)
 * (int64 [N]; candidates = L_b, or L_b - 1 without self loops).  Equal distances go to the lower j, as
 * np.argsort(kind='stable') orders them (the reference's default sort leaves ties unspecified).  A source without
 * candidates gets a key no pair reaches.  cgvp_graph_fill with these tau arrays then keeps key <= tau[i]. */
int cgvp_knn_graph_select(const float* ca_xyz, const int64_t* ptr, int64_t num_nodes, int64_t num_graphs, int32_t k,
                          int32_t keep_self_loops, double* tau_d2, int64_t* tau_j, int64_t* deg, void* stream);

/* edge_index [2][num_edges] int64: for every source i, its kept targets j in increasing order at positions
 * rowstart[i] ...; kept means |CA_i - CA_j|^2 <= radius^2 when tau_d2 == NULL (tau_j must be NULL too), else
 * (d2, j) <= (tau_d2[i], tau_j[i]) lexicographically (radius is ignored).  rowstart [N] int64.  A position outside
 * [0, num_edges) is not written, so a rowstart / num_edges that do not belong to these inputs cannot fault; entries
 * they leave uncovered keep their previous content. */
int cgvp_graph_fill(const float* ca_xyz, const int64_t* ptr, int64_t num_nodes, int64_t num_graphs, double radius,
                    const double* tau_d2, const int64_t* tau_j, int32_t keep_self_loops, const int64_t* rowstart,
                    int64_t num_edges, int64_t* edge_index, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CASTER_GVP_STRUCTURE_H */
