// The 'bf16' mode of the split-bf16 GEMM (gemm1x1s.hip with 1 bf16 part per operand) as a translation unit of its own.
#include "gemm1x1s_launch.h"
namespace dh { int launch_gemm1x1_split_p1(const ConvArgs& a, const ConvRoute& r, hipStream_t s) { return launch_split_parts<1>(a, r, s); } }
