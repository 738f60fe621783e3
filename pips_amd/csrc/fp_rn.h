// fp32 products, sums and differences that are rounded once and never fused.  hipcc's __fmul_rn / __fadd_rn / __fsub_rn are the
// plain operators, and the device default -ffp-contract=fast-honor-pragmas fuses a product with the sum that consumes it into one
// FMA wherever it sees the pair after inlining -- which product of `a b + c d` survives as a product is then the compiler's
// choice.  Where a rule states its arithmetic operation by operation and is held bit for bit to another implementation (the frame
// resize of pips_resize_frames and pips_frames_import and their torch twin), the operations come from here.
#pragma once
#include "common.h"

namespace pips {

__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

// the same in fp64 (the least-squares similarity of pips_motion_fit and its torch twin); a quotient is never fused
__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}

__device__ __forceinline__ double add_rn(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

__device__ __forceinline__ double sub_rn(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}

}  // namespace pips
