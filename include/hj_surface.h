/* libhj_surface.so: level sets of a stored value function as indexed meshes (gfx950).
 *
 * 2-D grids give oriented line segments, 3-D grids oriented triangles: marching simplices on the Kuhn (Freudenthal)
 * subdivision of every grid cell ("Level-set extraction").  The entry points are stateless, in the style of
 * hj_query.h: a plain grid descriptor (hjq_grid; bc / toward_zero / xlast are not read -- periodic axes are NOT wrapped)
 * and a HIP stream per call.  Every array pointer is DEVICE memory owned by the caller unless it says "host"; inputs are
 * never written; nothing is allocated and the device is never synchronised inside the library.  Return value: HJ_OK (0)
 * or a negative HJ_E* code of hj_mi355x.h; hjs_last_error() holds the text.
 *
 * Definition (the kernels and tests/surface_ref.py implement it to the bit):
 *   node      x_d(i) = xmin[d] + i*dx[d] in fp64, product and sum rounded separately
 *   inside    phi <= level (fp32 data converted to fp64 first); a simplex with a NaN / +-inf vertex emits nothing
 *   corner b  of a cell: bit d selects the upper node of axis d
 *   simplices of a cell: the permutations p of (0..D-1) in lexicographic order; v0 = 0, v_k = v_{k-1} | 1 << p[k-1]
 *   edge      corners a < b (as bit sets) of one cell; key = linear index of a's node * (2^D - 1) + ((b & ~a) - 1);
 *             active iff both ends are finite and exactly one is inside; every active edge carries one vertex at
 *             t = (level - phi_a) / (phi_b - phi_a) from a
 *   verts     nv x D fp64 in ascending key order
 *   faces     nf x D int32 (indices into verts), cells in ascending linear index, then simplex number; in 3-D the
 *             right-hand normal points toward increasing phi, in 2-D the inside lies to the left of p0 -> p1.
 *
 * Use: hjs_workspace_size -> hjs_count -> read counts back -> allocate verts / faces -> hjs_emit with the same
 * grid, data, level and workspace.
 */
#ifndef HJ_SURFACE_H
#define HJ_SURFACE_H
#include <stddef.h>
#include <stdint.h>
#include "hj_query.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of workspace hjs_count / hjs_emit need for nfields fields on grid g (about 6 bytes per node) */
int hjs_workspace_size(const hjq_grid* g, int64_t nfields, size_t* bytes);

/* Classify and scan.  data: nfields fields, field f at data + f*field_stride elements (dtype of the grid).
 * workspace: 8-byte aligned, at least hjs_workspace_size bytes.  counts: nfields x 2 int64, written as
 * (nv, nf) of every field.  ndim must be 2 or 3 (HJ_EUNSUPPORTED for 1 and 4), every N[d] >= 2, at most
 * 2^32 - 1024 nodes (HJ_EUNSUPPORTED beyond: hjs_emit runs one thread per node). */
int hjs_count(const hjq_grid* g, const void* data, int64_t nfields, int64_t field_stride, double level,
              void* workspace, size_t workspace_bytes, int64_t* counts, void* stream);

/* Write the meshes that hjs_count counted.  counts_host: HOST copy of hjs_count's counts (nfields x 2).  verts:
 * (sum of nv) x ndim fp64, faces: (sum of nf) x ndim int32, the fields one after the other; a field's face indices
 * count from that field's first vertex.  A field with nv or nf >= 2^31 gives HJ_EUNSUPPORTED; fields with
 * nv = nf = 0 launch nothing (verts / faces may then be null). */
int hjs_emit(const hjq_grid* g, const void* data, int64_t nfields, int64_t field_stride, double level,
             const void* workspace, size_t workspace_bytes, const int64_t* counts_host, double* verts,
             int32_t* faces, void* stream);

const char* hjs_last_error(void);
/* names of the kernels the calling thread's last successful call launched, in launch order, joined by ';', e.g.
 * "classify_kernel<double, 3>;scan_blocks_kernel"; hjs_emit lists emit_kernel once per field it launched for ("" when none) */
const char* hjs_last_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
