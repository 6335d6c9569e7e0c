// psvo C-ABI plumbing: thread-local error state and launch checking.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "psvo_common.h"
#include "lookback.h"
#include "query.h"

namespace psvo {

static thread_local char g_err[512] = "";
thread_local hipEvent_t g_stop_event = nullptr;
thread_local bool g_stop_share = false;
thread_local hipEvent_t g_stop_bound = nullptr;

int set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int check_launch(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PSVO_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return PSVO_OK;
}

// tests only: look-back controls for the sites in `mask` (lookback.h)
static int g_lb_debug_mask = 0, g_lb_debug_bound = -1, g_lb_debug_delay = 0;
LbCtl lb_ctl(int site) {
    const bool on = (g_lb_debug_mask & site) != 0;
    return LbCtl{on && g_lb_debug_bound >= 0 ? g_lb_debug_bound : kLbSpinMax, on ? g_lb_debug_delay : 0};
}

// the one-launch decoder backward's cost model (psvo_common.h bwd_split_na)
static BwdSplitCost g_bwd_split_cost = kBwdSplitCost;
BwdSplitCost bwd_split_cost() { return g_bwd_split_cost; }

}  // namespace psvo

// balance sweeps and tests: the cost model of the one-launch decoder backward
// (per-round costs a, b of class A / class B and class B's pre-loop cost b0;
// all 0: the built-in constants)
extern "C" int psvo_debug_set_bwd_split(int cost_a, int cost_b, int cost_b0) {
    if (cost_a == 0 && cost_b == 0 && cost_b0 == 0) {
        psvo::g_bwd_split_cost = psvo::kBwdSplitCost;
        return PSVO_OK;
    }
    PSVO_REQUIRE(cost_a >= 1 && cost_a <= 4096 && cost_b >= 1 && cost_b <= 4096 && cost_b0 >= 0 && cost_b0 <= 4096,
                 "debug_set_bwd_split: bad arguments");
    psvo::g_bwd_split_cost = psvo::BwdSplitCost{cost_a, cost_b, cost_b0};
    return PSVO_OK;
}

// tests: class A's workgroups of n_wg under the current cost model (-1: bad arguments)
extern "C" int psvo_debug_bwd_split(int64_t units_a, int64_t units_b, int n_wg) {
    if (units_a < 0 || units_b < 0 || n_wg < 1) return -1;
    return psvo::bwd_split_na(units_a, units_b, n_wg, psvo::bwd_split_cost());
}

extern "C" int psvo_debug_set_lookback(int mask, int spin_bound, int delay_us) {
    PSVO_REQUIRE(mask >= 0 && mask <= 7 && spin_bound >= -1 && delay_us >= 0 && delay_us <= 100000,
                 "debug_set_lookback: bad arguments");
    psvo::g_lb_debug_mask = mask;
    psvo::g_lb_debug_bound = spin_bound;
    psvo::g_lb_debug_delay = delay_us;
    return PSVO_OK;
}

extern "C" int psvo_debug_lb_helps(int64_t *out3, int reset) {
    PSVO_REQUIRE(out3, "debug_lb_helps: null argument");
    // {traversal, sampler, selection}: one counter per translation unit
    int rc = psvo::lb_helps_trace(out3, reset != 0);
    if (rc == PSVO_OK) rc = psvo::lb_helps_sample(out3 + 1, reset != 0);
    if (rc == PSVO_OK) rc = psvo::lb_helps_select(out3 + 2, reset != 0);
    return rc;
}

// tests only: the engine-internal selection / fused compositing entry points, arguments passed straight through
extern "C" int psvo_debug_select_samples(void *stream, int64_t r_hit, int s_max, float truncation, float max_depth,
                                         const int *offsets, const int *ray_ns, const float *z_vals, int z_stride,
                                         const int *rank_ray, const float *gt_depth, const float *sdf_s,
                                         const float *feat, const int *leaf, const float *t, const int *ray_of,
                                         int64_t cap, int split, int *cidx, int *offa, int *offb, float *feat_c,
                                         int *leaf_c, float *t_c, int *ray_of_c, float *rgb_c, int *src_c, int *counts,
                                         uint64_t *desc, uint32_t tag, int *host_flag) {
    return psvo::select_samples(psvo::as_stream(stream), r_hit, s_max, truncation, max_depth, offsets, ray_ns, z_vals,
                                z_stride, rank_ray, gt_depth, sdf_s, feat, leaf, t, ray_of, cap, split != 0, cidx, offa,
                                offb, feat_c, leaf_c, t_c, ray_of_c, rgb_c, src_c, counts,
                                reinterpret_cast<unsigned long long *>(desc), tag, host_flag);
}

extern "C" int64_t psvo_debug_select_granules(int64_t r_hit) { return psvo::select_granules(r_hit); }

extern "C" int psvo_debug_composite_loss(void *stream, int64_t r_hit, int s_max, float truncation, float max_depth,
                                         const int *offsets, const int *ray_ns, const float *z_vals, int z_stride,
                                         const int *rank_ray, const float *gt_rgb, const float *gt_depth,
                                         const float *sdf_s, const float *rgb_s, const float *coef, float *workspace,
                                         float *color, float *depth, float *grad_sdf_s, float *grad_rgb_s,
                                         int partials, const int *cidx) {
    return psvo::composite_loss_z(stream, r_hit, s_max, truncation, max_depth, offsets, ray_ns, z_vals, z_stride,
                                  rank_ray, gt_rgb, gt_depth, sdf_s, rgb_s, coef, workspace, color, depth, grad_sdf_s,
                                  grad_rgb_s, partials != 0, cidx);
}

extern "C" const char *psvo_last_error(void) { return psvo::g_err; }

extern "C" const char *psvo_version(void) { return "psvo 0.1.0 (gfx950)"; }
