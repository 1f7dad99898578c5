// The 'bf16x2' mode of the extended split-bf16 scope (gemm1x1s_ext.hip with 2 bf16 parts per operand) as a translation unit of its own.
#define DH_SPLIT_PARTS 2
#include "gemm1x1s_ext.hip"
