// The 'bf16' mode of the extended split-bf16 scope (gemm1x1s_ext.hip with 1 bf16 part per operand) as a translation unit of its own.
#include "gemm1x1s_ext_launch.h"
namespace dh { int launch_gemm1x1_split_ext_p1(const ConvArgs& a, const ConvRoute& r, hipStream_t s) { return launch_ext_parts<1>(a, r, s); } }
