/* include/gnf_dw_plan.h - a read-only view of the weight-gradient (dW) launch plan of the backward walk of libgnf_hip.so.
 * Included by gnf.h (which defines GnfMlp and the GNF_E* codes and opens the extern "C" block); not meant to be included on
 * its own. */
#ifndef GNF_DW_PLAN_H
#define GNF_DW_PLAN_H
#ifndef GNF_H
#error "include gnf.h, which includes this header"
#endif

/* Added within ABI v10 (new entry points only: no existing signature or struct changed, GNF_ABI_VERSION stays 10).
 * A DEBUGGING AND TEST VIEW, in the spirit of gnf_last_route: no stability promise - the record's layout follows the planner
 * and may change with it (out[0] is a layout version).  What gnf_grevnet_backward_f32 would decide for the weight gradients
 * of ONE half-step of n_nodes nodes of width D whose s- and t-net both have the shape of `net` (dims, attn; no pointer of it
 * is read, only whether attn / attn->Wo are NULL): the backward plan, the job list, the policy of the route and the cut, run
 * exactly as the walk runs them, on a never-dereferenced synthetic workspace base and synthetic gradient pointers, under the
 * library options set at the time of the call (dw_grouped, dw_wide_units, dw_thin_on_dw).  No device is touched: the CU count
 * the policies consult falls back to 256 without one, as in the size entry points.
 *   route       GNF_DW_ROUTE_STREAMS: the policy of the stream-forking route around a fused backward launch of bwd_tiles
 *               workgroups of bwd_lds bytes of LDS (0 / 0: no such launch - attention nets);  GNF_DW_ROUTE_GENERIC: the same
 *               route behind the generic GEMM backward (bwd_tiles, bwd_lds ignored);  GNF_DW_ROUTE_MERGED: the plan rides in
 *               the NEXT half-step's merged launch of bwd_tiles tile workgroups of bwd_lds bytes
 *   stashed     merged route: the walk reads the MLP-row stash (its tile workgroups have time for the thin jobs)
 *   last        merged route: the last half-step of the walk (its launch carries no tiles)
 *   slab_set    which of the plan's slab sets the launch writes (0; merged route: the parity of the step)
 *   accumulate  the gradients are added to (weight sharing)
 * out[0 .. return value): int64 fields, in this order (tests/golden/make_dw_plans.py names them the same way) -
 *   header (36): version n nj wide buf direct units lds maxred | plan_chunks plan_kchunk slab_chunks slab_sets slab_set wslab
 *                bslab slab_stride wsum osum | sk_q sk_steps sk_tiles sk_jobs sk_light_base xcd_jobs light_on_tiles
 *                unit_end | accumulate singles items | gx gy nz groups rpg blocks
 *                (buf: the buffer-load instance of whichever kernel runs; items: qpre[nj], the reduce's 16-byte items; the
 *                last six: the grouped kernel's geometry, 0 for a wide plan; the sk_ .. unit_end fields: 0 for a grouped one)
 *   per job, in launch order (13 each): job (its index in the half-step's job list) M N gx chunks kchunk unit_base lda ldb
 *                A B C aux
 *   per job, in job-list order (7 each): nw nb chunks wslab bslab gw gb     (the reduce's view)
 *   qpre[0 .. nj]
 * A pointer is written as its offset in floats from the workspace base, as -1 where it is NULL, or - where a slab was
 * redirected to the gradient itself - as the tag -(2 + 2 job + k), k = 0 the weight gradient, 1 the bias gradient of that job.
 * Returns the number of fields, or a negative GNF_E* code (GNF_EINVAL: a bad argument or cap too small - gnf_last_error tells
 * the count needed; GNF_EUNSUPPORTED as the walk would). */
enum GnfDwRoute { GNF_DW_ROUTE_STREAMS = 0, GNF_DW_ROUTE_MERGED = 1, GNF_DW_ROUTE_GENERIC = 2 };
#define GNF_DW_PLAN_RECORD_VERSION 1
int64_t gnf_dw_plan_describe(int64_t n_nodes, int32_t D, const GnfMlp* net, int32_t route, int64_t bwd_tiles, size_t bwd_lds,
                             int32_t stashed, int32_t last, int32_t slab_set, int32_t accumulate, int64_t* out, int64_t cap);

#endif /* GNF_DW_PLAN_H */
