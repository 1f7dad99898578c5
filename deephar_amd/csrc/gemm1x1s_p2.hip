// The 'bf16x2' mode of the split-bf16 GEMM (gemm1x1s.hip with 2 bf16 parts per operand) as a translation unit of its own.
#include "gemm1x1s_launch.h"
namespace dh { int launch_gemm1x1_split_p2(const ConvArgs& a, const ConvRoute& r, hipStream_t s) { return launch_split_parts<2>(a, r, s); } }
