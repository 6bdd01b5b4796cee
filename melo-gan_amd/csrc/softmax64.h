// The fp64 softmax of one row of fp32 logits, shared by the kernels that report the classifier's probabilities
// (morph_metrics.hip, mg_path_probs; roll_encode.hip, mg_window_votes), so that they cannot disagree about them.
#pragma once
#include "common.h"

// mg_cls_eval_acc's rule: the maximum (the lowest index on ties) is taken out and its own term, exp(0) = 1, is not computed;
// the other terms are added in class order.
__device__ __forceinline__ void softmax64_row(const float* __restrict__ z, int K, double* __restrict__ p) {
#pragma clang fp contract(off)
    int pred = 0;
    for (int k = 1; k < K; ++k)
        if (z[k] > z[pred]) pred = k;
    const double m = (double)z[pred];
    double rest = 0.0;
    for (int k = 0; k < K; ++k)
        if (k != pred) {
            const double e = exp((double)z[k] - m);
            p[k] = e;
            rest = rest + e;
        }
    const double sum = 1.0 + rest;
    for (int k = 0; k < K; ++k) p[k] = k == pred ? 1.0 / sum : p[k] / sum;
}
