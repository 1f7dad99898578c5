// The 'bf16x2' mode of the split-bf16 GEMM (gemm1x1s.hip with 2 bf16 parts per operand) as a translation unit of its own.
#define DH_SPLIT_PARTS 2
#include "gemm1x1s.hip"
