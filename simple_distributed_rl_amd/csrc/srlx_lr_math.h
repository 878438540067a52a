// srlx_lr_math.h -- the learning-rate schedules of LRSchedulerConfig.factor (srl/rl/schedulers/lr_scheduler.py:96-125; restated in
// simple_distributed_rl_amd/rl/schedulers/lr_scheduler.py:40-54) as ONE function for the host (srlx_lr_factor: what the CPU suite checks against the Python
// method) and the device (k_ppo_adam reads the optimiser's step count from device memory, so a captured update graph follows the schedule by itself).
// float64 throughout, the Python expression's order of operations (-ffp-contract=off): "step" = rate ** (step // decay_steps), "exp" = rate ** (step / decay_steps),
// "cosine" clamps step at decay_steps, "piecewise" counts the boundaries with step > b and returns values[k] / lr.  warmup_steps is not part of `factor`.
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "srlx.h"

namespace srlx {

__host__ __device__ inline bool lr_schedule_ok(const srlx_lr_schedule_t &s) {
    if (s.kind < SRLX_LR_CONSTANT || s.kind > SRLX_LR_PIECEWISE) return false;
    if ((s.kind == SRLX_LR_STEP || s.kind == SRLX_LR_EXP || s.kind == SRLX_LR_COSINE) && s.decay_steps <= 0) return false;
    if (s.kind == SRLX_LR_PIECEWISE && (s.n_boundaries < 0 || s.n_boundaries > SRLX_LR_MAX_BOUNDARIES)) return false;
    return true;
}

// Multiplier of the base rate `lr` at optimiser step `step` (0-based: the steps already taken)
__host__ __device__ inline double lr_factor(const srlx_lr_schedule_t &s, int64_t step, double lr) {
    switch (s.kind) {
    case SRLX_LR_STEP: {
        const int64_t k = step / s.decay_steps;  // (step >= 0: C's division is Python's //)
#if defined(__HIP_DEVICE_COMPILE__)
        // an integer power by repeated squaring: about 2 log2(k) multiplies where the library pow() is ~1000 instructions on the launch's critical path; within a
        // few ulp of pow() (exact for k <= 1, i.e. the whole first two stairs)
        double r = 1.0, x = s.decay_rate;
        for (int64_t n = k; n > 0; n >>= 1) {
            if (n & 1) r *= x;
            x *= x;
        }
        return r;
#else
        return pow(s.decay_rate, (double)k);  // (Python's float ** int is libm's pow: the same call)
#endif
    }
    case SRLX_LR_EXP:
        return pow(s.decay_rate, (double)step / (double)s.decay_steps);
    case SRLX_LR_COSINE: {
        const double alpha = s.min_lr / lr;
        const double x = (double)(step < s.decay_steps ? step : s.decay_steps) / (double)s.decay_steps;
        return (1.0 - alpha) * 0.5 * (1.0 + cos(3.141592653589793 * x)) + alpha;
    }
    case SRLX_LR_PIECEWISE: {
        int k = 0;
        for (int i = 0; i < SRLX_LR_MAX_BOUNDARIES; i++) k += (i < s.n_boundaries && step > s.boundaries[i]) ? 1 : 0;
        double v = s.values[0];
        for (int i = 1; i <= SRLX_LR_MAX_BOUNDARIES; i++) v = i == k ? s.values[i] : v;  // (selected without a run-time index into the kernel argument)
        return v / lr;
    }
    default:
        return 1.0;
    }
}

}  // namespace srlx
