/* ctd_hip_point_cloud.h -- the point-cloud family of libctd_hip.so: exact k-nearest-neighbours among bare points over a
 * sorted grid of cells, and the three small kernels that consume its lists (mean neighbour distance, covariance normals,
 * voxel means).  The mesh families answer "which face is near this point"; this one answers "which points are".
 *
 * An addition beside include/ctd_hip.h and the headers next to it (none of which includes it; ctd_version() is
 * unchanged): include what you call.  The status codes are those of ctd_hip.h; pointers are device pointers, `device`
 * and `stream` mean what they mean there.  One track per call; nothing here is differentiable.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * The grid.  A point p belongs to the cell with the coordinates
 *
 *   g_c = floorf((p_c - origin_c) / cell)      c = 0, 1, 2 (x, y, z), in f32, the division IEEE's
 *
 * when p is finite and 0 <= g_c < 2^21 for all three c (compared on the floats), and to no cell otherwise.  Its key is
 * the int64 g_0 + (g_1 << 21) + (g_2 << 42): x in the lowest bits, so the cells of an x-row are adjacent in key order.
 * A point of no cell has the key INT64_MAX.  The caller sorts the keys (stably, so that a cell's points stay in ascending
 * original index), and hands ctd_point_knn_f32 the sorted points, their original indices `order`, the unique keys
 * ascending and start[c], the position in the sorted points of the first point of unique cell c (start[n_cells] =
 * n_sorted).  There is no hash table: a neighbour cell is found by binary search in the unique keys.
 *
 * ctd_point_cell_keys_f32: keys[i] for points f32 [n][3]; one thread per point.
 *   CTD_ERR_INVALID_ARG for n < 0; for a cell that is not finite and > 0 or an origin that is not finite (a NaN fails);
 *   for a NULL points or keys when n > 0; for keys overlapping points.  n == 0 is CTD_OK.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_point_knn_f32 -- the rule.  For a finite query q and every point p of a cell, with the original index i:
 *
 *   dx = p_0 - q_0, dy = p_1 - q_1, dz = p_2 - q_2
 *   d2 = ((dx * dx) + (dy * dy)) + (dz * dz)         in f32, in that association, uncontracted
 *
 * p is a candidate when d2 <= max_d2 and d2 < +inf (max_d2 = +inf: no limit; the caller squares its distance once, as
 * f32).  The answer is the k candidates that come first in ascending (d2, i) order, the lower index winning a tie:
 * idx int32 [n_queries][k] and d2 f32 [n_queries][k].  Where fewer than k exist the rest are idx = -1, d2 = +inf.  A query
 * that is not finite has no neighbours.  This is the exact answer, bit-equal to brute force under the rule for every cell.
 *
 * queries == NULL: the points query themselves and n_queries is the number of entries of `order` (all points, those of
 * no cell after the n_sorted sorted ones).  Row order[t] is the list of sorted point t, from which the point itself is
 * excluded BY INDEX: a coincident other point stays, with d2 = 0.  The rows of the points of no cell are empty.
 * queries != NULL: row t belongs to queries[t]; nothing is excluded.
 *
 * The search.  A thread per query keeps the best K = 8, 16, 32 or 64 >= k candidates sorted in registers (a fully
 * unrolled insertion: no per-thread array is indexed at run time, so nothing goes to scratch).  The query's cell c is its
 * own g clamped into [0, dims).  It scans the block |g - c| <= 1, then one Chebyshev ring after the other, a row of
 * cells by one binary search.  After the block of radius r it stops when no unsearched cell can hold a candidate that
 * enters the list: an unsearched point has g_a >= c_a + r + 1 or g_a <= c_a - r - 1 on some axis a, which under the f32
 * rounding of g bounds its coordinate by origin_a + G * cell * (1 -+ 2^-22), G = c_a + r + 1 or c_a - r; the least such gap
 * to the query's own float coordinate, squared and shrunk by 2^-20 for the rounding of d2, is a lower bound of every
 * unsearched d2, and the search stops when the k-th d2 (or max_d2) is strictly below it, or when the block covers dims.
 * Without max_d2 a query far from every point therefore walks many empty rows.
 *
 *   CTD_ERR_INVALID_ARG for n_sorted < 0, n_cells < 0, n_queries < 0, n_cells > n_sorted or (n_cells == 0) !=
 *     (n_sorted == 0); for k outside [1, 64]; for a dim outside [1, 2^21]; for a cell that is not finite and > 0 or an
 *     origin that is not finite; for a max_d2 that is NaN or < 0;
 *   CTD_ERR_UNSUPPORTED for n_queries * k >= 2^31;
 *   CTD_ERR_INVALID_ARG for queries == NULL and n_queries < n_sorted; for a NULL idx or d2 when n_queries > 0; for a NULL
 *     sorted_points, order, keys or start when n_sorted > 0 (order also when queries == NULL and n_queries > 0); for idx
 *     or d2 overlapping each other or any input.
 * n_queries == 0 is CTD_OK.  One launch (more beyond 2^24 - 1 workgroups of 64 threads).
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_point_mean_dist_f32: per row of d2 f32 [n][k], the sum of sqrt((double)d2[j]) over the entries below +inf, in f64 in
 * list order, divided by their number and rounded to f32; NaN for a row without one.
 *   CTD_ERR_INVALID_ARG for n < 0, k outside [1, 64], a NULL pointer when n > 0, or mean overlapping d2;
 *   CTD_ERR_UNSUPPORTED for n * k >= 2^31.
 *
 * ctd_point_normals_f32: per point i of points f32 [n][3] with its row of idx int32 [n][k] (entries outside [0, n) are
 * skipped): the members are the point itself, then its neighbours in list order.  In f64: the centroid = (the members
 * summed in that order) / their number; then the six sums xx, xy, xz, yy, yz, zz of the products of (member - centroid),
 * in that order.  A cyclic Jacobi of 10 fixed sweeps gives the eigenvalues l0 <= l1 <= l2 and the unit eigenvector of l0,
 * rounded to f32: normals f32 [n][3]; variation f32 [n] = l0 / ((l0 + l1) + l2); ok u8 [n] = 0, with NaN normal and
 * variation, for fewer than 3 members or l1 - l0 <= 1e-9 * l2 (a line, a single point, an isotropic blob).  toward != NULL:
 * f32, toward_stride = 0 (one viewpoint) or 3 (one per point); the normal is negated where
 * ((n_0 * v_0) + (n_1 * v_1)) + (n_2 * v_2) < 0, v = toward - p in f64, before it is rounded.  cov != NULL: f64 [n][9], the
 * centroid and the six sums.
 *   CTD_ERR_INVALID_ARG for n < 0, k outside [1, 64], a toward_stride other than 0 or 3, a NULL points, idx, normals,
 *     variation or ok when n > 0, or an output overlapping an input or another output; CTD_ERR_UNSUPPORTED for
 *     n * k >= 2^31.
 *
 * ctd_point_voxel_mean_f32: out f32 [n_cells][C]; row c, column j is the f64 sum of values[order[s]][j] for s = start[c] ..
 * start[c + 1] - 1, in that order (ascending original index after a stable sort), divided by the count, rounded to f32
 * once.  values f32 [n][C]; entries of order outside [0, n) are skipped.
 *   CTD_ERR_INVALID_ARG for n < 0, n_cells < 0, C outside [1, 64], a NULL pointer when n_cells > 0, or out overlapping
 *     an input; CTD_ERR_UNSUPPORTED for n * C or n_cells * C >= 2^31.
 *
 * Every check happens before any HIP call.  All stores are plain vector stores; no atomics, no workspace.
 */
#ifndef CTD_HIP_POINT_CLOUD_H
#define CTD_HIP_POINT_CLOUD_H

#include "../ctd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int ctd_point_cell_keys_f32(const float* points, int n, float origin_x, float origin_y, float origin_z, float cell,
                            int64_t* keys, int device, void* stream);

int ctd_point_knn_f32(const float* sorted_points, const int32_t* order, int n_sorted, const int64_t* keys,
                      const int32_t* start, int n_cells, int dim_x, int dim_y, int dim_z, float origin_x, float origin_y,
                      float origin_z, float cell, const float* queries, int n_queries, int k, float max_d2, int32_t* idx,
                      float* d2, int device, void* stream);

int ctd_point_mean_dist_f32(const float* d2, int n, int k, float* mean, int device, void* stream);

int ctd_point_normals_f32(const float* points, int n, const int32_t* idx, int k, const float* toward, int toward_stride,
                          float* normals, float* variation, uint8_t* ok, double* cov, int device, void* stream);

int ctd_point_voxel_mean_f32(const float* values, int n, int C, const int32_t* order, const int32_t* start, int n_cells,
                             float* out, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_POINT_CLOUD_H */
