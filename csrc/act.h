// Activations of the GEMM epilogues (gemm.hip, gemm_f32.hip): the codes of the C ABI's `act` / `dact`
// arguments, the activation, and its derivative expressed through the saved layer output.
#pragma once

#include "common.h"

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_SIGMOID = 2, ACT_TANH = 3 };

EM_DEVICE float act_fn(float x, int act) {
  switch (act) {
    case ACT_RELU: return fmaxf(x, 0.f);
    case ACT_SIGMOID: return 1.f / (1.f + __expf(-x));
    case ACT_TANH: return tanhf(x);
    default: return x;
  }
}

// act'(z) from the saved output y = act(z).  A code that is none of the three activations means tanh to
// the bf16 kernels (their callers pass 1 .. 3 only) and, with none_is_one, the identity's derivative 1 to
// gemm_f32.hip, where "none" is a valid code.
EM_DEVICE float act_dfn(float y, int act, bool none_is_one = false) {
  if (act == ACT_RELU) return y > 0.f ? 1.f : 0.f;
  if (act == ACT_SIGMOID) return y * (1.f - y);
  if (none_is_one && act != ACT_TANH) return 1.f;
  return 1.f - y * y;
}
