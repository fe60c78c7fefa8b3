// Integer helpers of the host code (no HIP): shared by xg_common.h and the GEMM planner (xg_gemm_route.h).
#pragma once
#include <stdint.h>

static inline int xg_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int64_t xg_cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
