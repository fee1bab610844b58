/*
 * s2d_debug.h - debugging / tuning entries of libs2d_hip.so.  NOT part of the drop-in boundary (include/s2d.h): nothing in the reference
 * binds them; they exist for tools/side_stress.py and tools/spconv_kernel_bench.py and may change without notice.
 */
#ifndef S2D_DEBUG_H
#define S2D_DEBUG_H

#include "s2d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* debugging aid (no reference counterpart): `blocks` workgroups fill 64 KB of LDS each with `value`, `spin` + 1 times; sink may be NULL.
 * tools/side_stress.py uses it to look for kernels that read LDS they did not write. */
int s2d_debug_lds_fill(float value, int blocks, int spin, float *sink, s2d_stream_t stream);

/* tuning aid (tools/spconv_kernel_bench.py --trace): device buffer int64[grid][64] that the ablation build of the register-gather
 * kernel (csrc/spconv_rg.hip) fills with per-step s_memtime stamps when S2D_RG_DEBUG has bit 32 set; NULL switches it off */
void s2d_debug_rg_trace(void *buf);

/* test / tuning aids of the dense 2-D tile kernels (csrc/conv2d_nhwc.hip; tests/test_conv2d_parity_gpu.py sweeps every instantiation in one
 * process with them).  The launch plan follows S2D_CONV_BM / S2D_CONV_NS / S2D_CONV_SHARED_A / S2D_CONV1X1, read from the environment
 * at first use; s2d_conv2d_debug_force overrides them for all launches AND plan queries that follow: bm = rows per tile of the 32-deep
 * kernel (64, 96, 128), ns = 32 (the 32-deep kernel) or 2, 3, 4 (the 64-deep ring of that depth, 3x3 entries), shared_a = 0 / 1 (the
 * tap-shared pad-1 stride-1 3x3 kernel), conv1x1_k64 = 0 / 1 (1x1 launches on the 64-deep double buffer); -1 = as the environment says.
 * Callers that sized a statistics buffer with a *_stats_tiles query must not change the plan between the query and the launch (the
 * Python package memoises those queries: force only around raw-pointer calls, and restore with (-1, -1, -1, -1)). */
int s2d_conv2d_debug_force(int bm, int ns, int shared_a, int conv1x1_k64);

/* the launch plan an entry takes for these arguments - the function the launchers and the *_stats_tiles / *_tile_rows /
 * *_bnbwd_supported queries read.  kind: 0 conv2d3x3, 1 conv2d3x3 bnbwd, 2 conv2d1x1, 3 conv2d1x1 bnbwd, 4 convup, 5 conv2d4x4s2,
 * 6 conv2d2x2s2; (n, h, w, cin, cout) as the entry takes them (convup: source grid, kc, nc); pad / stride: the 3x3 kinds; ks: convup.
 * out = {kernel family (0 the 32-deep kernel, 1 the 64-deep ring, 2 shared-A), BN, rows per tile, NS, grid x, y, z, statistics
 * slabs (row tiles; convup: 4 x row tiles, slab = class * row tiles + tile)}.  Returns S2D_ERR_UNSUPPORTED (out still filled where
 * the geometry is valid) for shapes or epilogues the entry refuses.  No device work. */
int s2d_conv2d_plan(int kind, int n, int h, int w, int cin, int cout, int pad, int stride, int ks, int32_t out[8]);

/* test / tuning aids of the dense 2-D weight-gradient kernels (csrc/conv2d_wgrad.hip; tests/test_conv2d_wgrad_parity_gpu.py sweeps every
 * instantiation and K-loop length in one process with them).  ring_deep = 0 / 1: the four-slot LDS ring / as many slots as fit (what
 * S2D_WG_RING_DEEP, read from the environment at first use, selects); splits >= 1 replaces the term CUs / (grid y * channel tiles) of the
 * split count before its clamps (at most one split per K-step; the count is then re-derived from the rounded-up steps per workgroup);
 * -1 = as the environment / the CU count says.  Overrides all launches AND *_wgrad_workspace_bytes queries that follow (the Python
 * package memoises those queries: force only around raw-pointer calls, and restore with (-1, -1)).  Any other value: S2D_ERR_INVALID_ARG,
 * nothing changed. */
int s2d_conv2d_wgrad_debug_force(int ring_deep, int splits);

/* the launch plan a weight-gradient entry takes for these arguments - the function the launchers and the three *_wgrad_workspace_bytes
 * queries read.  kind: 0 conv2d3x3_wgrad (ks 3), 1 conv2d1x1_wgrad (ks 1, pad 0), 2 conv2d_s2_wgrad (ks 3 or 4, pad 1); (n, h, w) as the
 * entry takes them; c_in_role = channels of the tensor the taps walk over (cin; cb of the stride-2 entry), c_out_role = of the other
 * (cout; ca).  out = {TCO, TCI, NS (LDS ring slots), KXN (kx taps per workgroup), splits, K-steps per workgroup, grid y, grid z}.
 * Returns S2D_ERR_UNSUPPORTED for shapes the entry refuses.  No device work. */
int s2d_conv2d_wgrad_plan(int kind, int n, int h, int w, int c_in_role, int c_out_role, int pad, int ks, int32_t out[8]);

#ifdef __cplusplus
}
#endif

#endif /* S2D_DEBUG_H */
