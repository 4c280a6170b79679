// The per-element arithmetic of torch.optim.SGD (no momentum), torch.optim.Adagrad (lr_decay = 0) and torch.optim.RMSprop (not
// centered, no momentum): the single-tensor paths, one function per optimizer, beside cdr_adam_math.h.  Floating-point contraction
// is OFF inside: every operation rounds on its own, in torch's order, so every kernel that calls one of these gets the same bits from
// the same operands whatever the compiler does around the call.
//
// Square root and division are the IEEE-correct sqrtf and `/` (NOT v_sqrt_f32 / v_rcp_f32 as in cdr_adam_term): none of these
// optimizers has a per-row replay that is VALU-bound (cdr_adam_math.h, round 4, was about lz_prepare_kernel), the dense sweep moves
// 16-20 B per element and hides ~25 more instructions, and with IEEE operations the fp32 result of one update is torch's own.
#pragma once
#include <hip/hip_runtime.h>

// THE Adagrad / RMSprop update term:   lr * g / (sqrt(s) + eps)      torch: std = s.sqrt().add_(eps); p.addcdiv_(g, std, value=-lr)
__device__ __forceinline__ float cdr_rootsum_term(float gv, float sv, float lr, float eps) {
#pragma clang fp contract(off)
    const float denom = sqrtf(sv) + eps;
    return lr * (gv / denom);
}

//   g += wd*p ; p -= lr g                                            torch.optim.SGD(momentum=0)
__device__ __forceinline__ float cdr_sgd_elem(float pv, float gv, float lr, float wd) {
#pragma clang fp contract(off)
    if (wd != 0.f) gv = gv + wd * pv;
    return pv - lr * gv;
}

//   g += wd*p ; s += g g ; p -= cdr_rootsum_term(g, s)               torch.optim.Adagrad(lr_decay=0): eps = 1e-10 by default
// A zero gradient with wd == 0 leaves s and p bit for bit (s + 0 = s, p - lr * (0 / (sqrt(s) + eps)) = p - 0): the row-wise form of
// this optimizer IS the dense one.
__device__ __forceinline__ float cdr_adagrad_elem(float pv, float gv, float& s, float lr, float eps, float wd) {
#pragma clang fp contract(off)
    if (wd != 0.f) gv = gv + wd * pv;
    const float sv = s + gv * gv;                          // state_sum.addcmul_(grad, grad, value=1)
    s = sv;
    return pv - cdr_rootsum_term(gv, sv, lr, eps);
}

//   g += wd*p ; v = alpha v + (1 - alpha) g g ; p -= cdr_rootsum_term(g, v)      torch.optim.RMSprop: alpha = 0.99, eps = 1e-8
// `oma` is 1 - alpha rounded ONCE from the caller's double (torch hands addcmul_ the Python float 1 - alpha; 1.0f - (float)alpha is
// 1e-6 away from it at alpha = 0.99).
__device__ __forceinline__ float cdr_rmsprop_elem(float pv, float gv, float& v, float lr, float alpha, float oma, float eps, float wd) {
#pragma clang fp contract(off)
    if (wd != 0.f) gv = gv + wd * pv;
    const float vv = alpha * v + (oma * gv) * gv;          // square_avg.mul_(alpha).addcmul_(grad, grad, value=1 - alpha)
    v = vv;
    return pv - cdr_rootsum_term(gv, vv, lr, eps);
}
