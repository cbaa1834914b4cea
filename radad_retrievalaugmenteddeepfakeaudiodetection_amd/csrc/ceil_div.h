// ceil_div.h -- the one integer helper that host-only headers (knn_plan.h) and common.h share.
#pragma once
#include <stdint.h>

static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }
