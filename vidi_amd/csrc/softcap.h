// The final-logit softcap (gemma.py:565-569) as ONE expression: T(T(tanh(T(x / cap))) * cap), every module output rounded where eager PyTorch
// rounds.  elementwise.hip (softcap + argmax, in place) and vocab_logprob.hip (log-probabilities, read-only) include it, so both see the same
// bits.  (A header of its own: common.h and kernels.h belong to the digest that keys the GEMM family's PMC traffic record.)
#pragma once
#include "common.h"

template <typename T>
__device__ __forceinline__ float softcap_value(float x, float cap) { return rnd<T>(rnd<T>(tanhf(rnd<T>(x / cap))) * cap); }
