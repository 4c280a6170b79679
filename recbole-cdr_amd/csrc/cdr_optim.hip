// config['learner'] beyond Adam (recbole Trainer._build_optimizer: sgd / adagrad / rmsprop with torch's defaults): the dense sweep of
// torch.optim.SGD, Adagrad and RMSprop over MANY parameter tensors in one launch, in the style of cdr_adam_multi_dev (cdr_rows.hip).
// HBM-bound: 12 B (SGD) / 20 B (Adagrad, RMSprop) per element, 16-B requests where the tensors allow, a grid stride beyond 8 blocks per
// CU and tensor.  None of the three has a bias correction, so there is no step counter on the device and nothing for the launch to wait
// for: it is capturable as it stands.  The arithmetic is cdr_opt_math.h's, one function per optimizer.
#include "cdr_common.h"
#include "cdr_opt_math.h"

namespace {

inline int grid_cap(int64_t blocks) {
    const int64_t cap = CDR_NUM_CU * 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

constexpr int kOptMulti = 24;
struct opt_multi_args {
    float* p[kOptMulti];
    const float* g[kOptMulti];
    float* s[kOptMulti];            // Adagrad: sum; RMSprop: square_avg; SGD: unused (NULL)
    int64_t n[kOptMulti];
    int blk_start[kOptMulti + 1];
    int count;
};
struct opt_hp { float lr, alpha, oma, eps, wd; };

template <int OPT>
__device__ __forceinline__ float opt_elem(float pv, float gv, float& sv, const opt_hp& h) {
    if constexpr (OPT == CDR_OPT_SGD) return cdr_sgd_elem(pv, gv, h.lr, h.wd);
    else if constexpr (OPT == CDR_OPT_ADAGRAD) return cdr_adagrad_elem(pv, gv, sv, h.lr, h.eps, h.wd);
    else return cdr_rmsprop_elem(pv, gv, sv, h.lr, h.alpha, h.oma, h.eps, h.wd);
}

template <int OPT>
__global__ __launch_bounds__(kBlock) void opt_multi_kernel(opt_multi_args a, opt_hp h, const float* __restrict__ loss,
                                                           float* __restrict__ loss_sum) {
    constexpr bool STATE = OPT != CDR_OPT_SGD;
    // the epoch's loss total (recbole Trainer._train_epoch: total_loss += loss.item()) rides in this launch: nothing else in it touches
    // the two words, and launches on one stream are ordered, so one thread's read-modify-write is the whole of it
    if (loss_sum && blockIdx.x == 0 && threadIdx.x == 0) loss_sum[0] += loss[0];
    int t = 0;
    while (t + 1 < a.count && (int)blockIdx.x >= a.blk_start[t + 1]) ++t;
    const int nb = a.blk_start[t + 1] - a.blk_start[t], lb = (int)blockIdx.x - a.blk_start[t];
    float* __restrict__ p = a.p[t];
    const float* __restrict__ g = a.g[t];
    float* __restrict__ s = a.s[t];
    const int64_t n = a.n[t];
    const int64_t stride = (int64_t)nb * kBlock;
    const bool vec16 = !(n & 3) && !(((uintptr_t)p | (uintptr_t)g | (STATE ? (uintptr_t)s : 0)) & 15);
    if (vec16) {           // 16-B requests
        const int64_t n4 = n >> 2;
        for (int64_t e = (int64_t)lb * kBlock + threadIdx.x; e < n4; e += stride) {
            float4 pv = ld4(p + 4 * e), sv = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (STATE) sv = ld4(s + 4 * e);
            const float4 gv = ld4(g + 4 * e);
            pv.x = opt_elem<OPT>(pv.x, gv.x, sv.x, h);
            pv.y = opt_elem<OPT>(pv.y, gv.y, sv.y, h);
            pv.z = opt_elem<OPT>(pv.z, gv.z, sv.z, h);
            pv.w = opt_elem<OPT>(pv.w, gv.w, sv.w, h);
            st4(p + 4 * e, pv);
            if constexpr (STATE) st4(s + 4 * e, sv);
        }
        return;
    }
    for (int64_t e = (int64_t)lb * kBlock + threadIdx.x; e < n; e += stride) {
        float sv = 0.f;
        if constexpr (STATE) sv = s[e];
        p[e] = opt_elem<OPT>(p[e], g[e], sv, h);
        if constexpr (STATE) s[e] = sv;
    }
}

}  // namespace

extern "C" int cdr_opt_multi_dev(void* stream, int opt, int count, float* const* params, const float* const* grads, float* const* state,
                                 const int64_t* numel, float lr, double alpha, float eps, float weight_decay, const float* loss,
                                 float* loss_sum) {
    CDR_CHECK_ARG(opt == CDR_OPT_SGD || opt == CDR_OPT_ADAGRAD || opt == CDR_OPT_RMSPROP);      // (Adam: cdr_adam_multi_dev)
    CDR_CHECK_ARG(count > 0 && params && grads && numel);
    CDR_CHECK_ARG(opt == CDR_OPT_SGD || state);
    CDR_CHECK_ARG((loss == nullptr) == (loss_sum == nullptr));
    for (int j = 0; j < count; ++j) CDR_CHECK_ARG(params[j] && grads[j] && numel[j] > 0 && (opt == CDR_OPT_SGD || state[j]));
    hipStream_t s = (hipStream_t)stream;
    const opt_hp h{lr, (float)alpha, (float)(1.0 - alpha), eps, weight_decay};
    for (int base = 0; base < count; base += kOptMulti) {
        opt_multi_args a{};
        a.count = count - base < kOptMulti ? count - base : kOptMulti;
        int blocks = 0;
        for (int i = 0; i < a.count; ++i) {
            const int j = base + i;
            a.p[i] = params[j]; a.g[i] = grads[j]; a.s[i] = opt == CDR_OPT_SGD ? nullptr : state[j]; a.n[i] = numel[j];
            a.blk_start[i] = blocks;
            blocks += grid_cap((numel[j] + kBlock * 4 - 1) / (kBlock * 4));      // ~4 elements per thread, capped per tensor
        }
        a.blk_start[a.count] = blocks;
        const float* l = base == 0 ? loss : nullptr;
        float* ls = base == 0 ? loss_sum : nullptr;
        if (opt == CDR_OPT_SGD) opt_multi_kernel<CDR_OPT_SGD><<<dim3(blocks), dim3(kBlock), 0, s>>>(a, h, l, ls);
        else if (opt == CDR_OPT_ADAGRAD) opt_multi_kernel<CDR_OPT_ADAGRAD><<<dim3(blocks), dim3(kBlock), 0, s>>>(a, h, l, ls);
        else opt_multi_kernel<CDR_OPT_RMSPROP><<<dim3(blocks), dim3(kBlock), 0, s>>>(a, h, l, ls);
        CDR_LAUNCH_CHECK();
    }
    return CDR_OK;
}
