// The loss arithmetic of the row-wise family (cdr_step.hip, cdr_kstep.hip, cdr_dimshard.hip, cdr_gather_loss.hip; cdr_ordered.hip mirrors
// the EmbLoss coefficient) and the hand-over of a block's partial sums.  Every route that the suite compares bit for bit -- count path
// against sorted path, dimension and row shards against the fused step, k-major against per-row, dense against row-wise -- calls these
// functions: a loss term is never restated in a kernel.  (cdr_conet.hip accumulates its BCE in double and keeps its own two lines.)
#pragma once
#include "cdr_common.h"

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// recbole's BPRLoss on the score difference x = <u,p> - <u,n>, with s = sigmoid(x): one term -log(gamma + s) of the batch mean, and
// g = d(mean)/dx.  Two functions so that a kernel can take the logarithm in its loss lane only; bpr_term is both at one place
__device__ __forceinline__ float bpr_loss(float s, float gamma) { return -logf(gamma + s); }
__device__ __forceinline__ float bpr_grad(float s, float gamma, float invB) { return -invB * (s * (1.0f - s)) / (gamma + s); }
__device__ __forceinline__ void bpr_term(float x, float gamma, float invB, float& loss, float& g) {
    const float s = sigmoidf_(x);
    g = bpr_grad(s, gamma, invB);
    loss = bpr_loss(s, gamma);
}

// One row of torch's MSELoss on the raw dot dx, or of BCELoss on p = sigmoid(dx) with its -100 clamp of both logs and its backward
// (p - y) / max((1 - p) p, 1e-12); g = d(mean)/d(dx); score = what the model reports for the row (dx resp. p)
__device__ __forceinline__ void point_term(int loss_kind, float dx, float y, float invB, float& loss, float& g, float& score) {
    if (loss_kind == CDR_LOSS_MSE) {
        const float d = dx - y;
        loss = d * d; g = 2.0f * d * invB; score = dx;
    } else {
        const float p = sigmoidf_(dx);
        loss = (y - 1.0f) * fmaxf(logf(1.0f - p), -100.0f) - y * fmaxf(logf(p), -100.0f);
        const float pq = (1.0f - p) * p;
        g = (p - y) / fmaxf(pq, 1e-12f) * invB * pq; score = p;
    }
}
__device__ __forceinline__ void point_term(int loss_kind, float dx, float y, float invB, float& loss, float& g) {
    float score;
    point_term(loss_kind, dx, y, invB, loss, g, score);
}

// recbole's EmbLoss reg_weight * ||W_b||_2 / B: its gradient is c * W_b with c = reg_weight / (B * norm); 0 without EmbLoss or for a zero
// norm (torch.norm's backward there).  k: rows of the batch one list occurrence stands for (k-major lists)
__device__ __forceinline__ float embloss_coef(float reg_weight, int64_t B, float norm, float k = 1.0f) {
    return (reg_weight != 0.f && norm > 0.f) ? k * (reg_weight / ((float)B * norm)) : 0.f;
}

// SSCDR's metric loss, per element (sscdr.py:120-128, 142-144): the squared-norm "normalize" divides a row by L = sum x^2 where L > 1
// (the SQUARED length: the reference's quirk, kept) -- sqnorm_scale is that divisor, the arithmetic of sqnorm_normalize_fwd_kernel --
// and nn.TripletMarginLoss(p=2, eps) on the normalised rows.  unit_dir: one element of d(distance)/d(difference) of a triple whose
// hinge is open (`on`), 0 for a closed hinge or a zero distance -- triplet_bwd_kernel's and sscdr_map_loss_kernel's conventions.
// sqnorm_bwd_elem: one element of the gradient taken back through the normalisation, g the gradient at the normalised element and
// dot = <x, g> over the row -- sq_norm_bwd of cdr_elem.hip (sqnorm_normalize_bwd_kernel).
__device__ __forceinline__ float sqnorm_scale(float L) { return L > 1.0f ? L : 1.0f; }
__device__ __forceinline__ float unit_dir(bool on, float diff, float dist) { return (on && dist > 0.f) ? diff / dist : 0.f; }
__device__ __forceinline__ float sqnorm_bwd_elem(float x, float g, float L, float dot) { return L > 1.0f ? g / L - (2.0f * dot / (L * L)) * x : g; }
// One term of the hinge's batch sum, and whether it is open
__device__ __forceinline__ float triplet_hinge(float d1, float d2, float margin, bool& on) {
    const float h = d1 - d2 + margin;
    on = h > 0.0f;
    return fmaxf(h, 0.0f);
}

// Thread 0, after block_sum_d<N>: the block's N sums into its slot of cdr_ctx::partials.  _sys: past the L2s, for cdr_sign_in_last
template <int N>
__device__ __forceinline__ void store_partials(double* partials, const double (&acc)[N]) {
    double* o = partials + (size_t)blockIdx.x * CDR_PARTIAL_STRIDE;
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = acc[i];
}
template <int N>
__device__ __forceinline__ void store_partials_sys(double* partials, const double (&acc)[N]) {
    double* o = partials + (size_t)blockIdx.x * CDR_PARTIAL_STRIDE;
#pragma unroll
    for (int i = 0; i < N; ++i) cdr_store_sys(o + i, acc[i]);
}

// A finishing block of BLOCK threads: the N sums over the nblocks slots that store_partials filled (thread t adds slots t, t + BLOCK, ...
// in that order, then block_sum_d<N>), valid in thread 0.  BLOCK is the launch's block size as a constant -- read from blockDim.x the loop
// compiles to other code.  SYS: the slots were written by store_partials_sys and are read past the L2s.
template <int N, int BLOCK, bool SYS = false>
__device__ __forceinline__ void sum_partials(const double* partials, int nblocks, double (&acc)[N], double* smem) {
    for (int b = threadIdx.x; b < nblocks; b += BLOCK) {
        const double* o = partials + (size_t)b * CDR_PARTIAL_STRIDE;
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] += SYS ? cdr_load_sys(o + i) : o[i];
    }
    block_sum_d<N>(acc, smem);
}

__device__ __forceinline__ float4 scale4(float g, float4 a) { return make_float4(g * a.x, g * a.y, g * a.z, g * a.w); }
__device__ __forceinline__ float4 neg4(float4 a) { return make_float4(0.f - a.x, 0.f - a.y, 0.f - a.z, 0.f - a.w); }
__device__ __forceinline__ float4 neg_scale4(float g, float4 a) { return neg4(scale4(g, a)); }
__device__ __forceinline__ float4 scale_diff4(float g, float4 a, float4 b) { return make_float4(g * (a.x - b.x), g * (a.y - b.y), g * (a.z - b.z), g * (a.w - b.w)); }
