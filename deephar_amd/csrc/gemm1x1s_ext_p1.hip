// The 'bf16' mode of the extended split-bf16 scope (gemm1x1s_ext.hip with 1 bf16 part per operand) as a translation unit of its own.
#define DH_SPLIT_PARTS 1
#include "gemm1x1s_ext.hip"
