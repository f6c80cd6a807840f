/*
 * srt_query_sort.h -- coherence-sorted ray queries: srt_query_closest and srt_query_occluded with the rays traced in
 * an order in which neighbouring lanes walk neighbouring nodes.
 *
 * A ray's answer does not depend on which lane traced it, so every result is bit-identical to the unsorted call's:
 * rays are read and results written in place, hits_dev[i] belongs to rays_dev[i].  Only the order of the work changes.
 * The order is built on the device in front of the traversal -- the bounds of the origins, a key per ray, a radix
 * sort -- and costs its own time: it pays for rays that arrive incoherent (started on surfaces, say) and loses on
 * rays that arrive coherent (a camera's); DESIGN.md section 5, "Sorted ray queries", has the measurements.
 *
 * The rule (csrc/ray_order_rule.hpp is its text, compiled for the device and for srt_ray_order):
 *   1. per axis, lo and hi are the least and greatest origin[k] over the rays whose origin[k] is finite (-0 below +0);
 *      an axis without a finite origin has lo = hi = 0;
 *   2. origin cell: ext = hi - lo; u = ext > 0 ? ((o - lo) / ext) * 2^origin_bits : 0; the cell is 0 unless u > 0,
 *      2^origin_bits - 1 from there up, else u truncated (a NaN gives 0);
 *   3. direction cell: m = max(|dx|, |dy|, |dz|); u = (d[k] / m + 1) * 2^(dir_bits - 1) where 0 < m <= FLT_MAX, else
 *      0; converted the same way;
 *   4. key = (Morton(origin cells) << 3 * dir_bits) | Morton(direction cells), x the most significant of each triple;
 *   5. the order is the stable sort of 0 .. n-1 by key: rays with equal keys keep the caller's order.
 * All arithmetic is single fp32 operations, uncontracted.  srt_query_get_int: "sort.origin_bits" and "sort.dir_bits"
 * (the two bit counts per axis), "sort.bytes" (scratch held for sorting: 16 B a ray, the sort's temporary storage, the
 * bounds), "sort.launches" (launches of the last sorted call -- bounds, keys, the sort counted as one, the traversal,
 * and on a rebuilt object closest's triangle remap; 0 before any), "sort.count" (sorted calls so far that launched).
 *
 * Additive to srt_query.h (SRT_QUERY_ABI_VERSION is unchanged); versioned on its own.
 */
#ifndef SRT_QUERY_SORT_H
#define SRT_QUERY_SORT_H

#include "srt_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_QUERY_SORT_ABI_VERSION 1

int srt_query_sort_abi_version(void);                              /* 1 */
/* srt_query_closest / srt_query_occluded through the sorted order.  Both only enqueue on the query's stream: no
 * synchronisation, no host copy, and no allocation at a steady n (the scratch is held in the object and grown only
 * when n grows).  n == 0 is SRT_OK and launches nothing; n > INT_MAX is SRT_ERR_INVALID (the device sort counts in
 * int); NULL or misaligned pointers fail as the unsorted calls fail. */
int srt_query_closest_sorted (srt_query* q, const srt_ray* rays_dev, uint32_t n, srt_hit*  hits_dev);
int srt_query_occluded_sorted(srt_query* q, const srt_ray* rays_dev, uint32_t n, uint8_t* occluded_dev);
/* host mirror of the rule: order[n]; keys[n] and bounds[6] optional (NULL skips).  keys[i] is the key of ray
 * order[i]; bounds is lo xyz, hi xyz.  HOST pointers; no device is touched. */
int srt_ray_order(const srt_ray* rays, uint32_t n, uint32_t* order, uint32_t* keys, float* bounds);
/* test and debug readback of the LAST sorted call's permutation and sorted keys; synchronises; NULL skips;
   SRT_ERR_STATE when no sorted call has run or n differs from that call's */
int srt_query_copy_ray_order(srt_query* q, uint32_t* order, uint32_t* keys, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif
