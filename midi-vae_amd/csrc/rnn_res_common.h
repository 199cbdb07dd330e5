// Device helpers shared by the resident recurrent kernels: one wave per SIMD (rnn_resident.hip), two waves per SIMD (rnn_w8.hip).
#pragma once
#include "common.h"
#include <type_traits>

namespace {

typedef u16x8 frag;          // one lane's 16 bytes of an MFMA operand fragment (8 bf16)
enum { SAVE_NONE = 0, SAVE_HS = 1, SAVE_ALL = 2 };

// Compile-time loop: f(std::integral_constant<int, i>) for i = I .. N-1, so that slot numbers are constants for `if constexpr`
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
#define SF_LAMBDA(ic) [&](auto ic) __attribute__((always_inline))

// One MFMA as its own asm statement (a slot); A operand in accumulator registers (AG) or vector registers
template <bool AG>
__device__ __forceinline__ void mfma1(f32x4& c, const frag& u, const frag& b) {
    if (AG) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "a"(u), "v"(b));
    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(u), "v"(b));
}
__device__ __forceinline__ void vm_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// Empty volatile statements: tie a loaded register to the wait in front of it / keep a value where it is
__device__ __forceinline__ void pin1(u16x4& a) { asm volatile("" : "+v"(a)); }
__device__ __forceinline__ void pini(int& a) { asm volatile("" : "+v"(a)); }
__device__ __forceinline__ void pinu(unsigned& v) { asm volatile("" : "+v"(v)); }

__device__ __forceinline__ u16x8 cat8(u16x4 a, u16x4 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }
__device__ __forceinline__ f32x4 unpack4(u16x4 p) { return f32x4{bf2f(p[0]), bf2f(p[1]), bf2f(p[2]), bf2f(p[3])}; }
__device__ __forceinline__ u16x4 pack4(f32x4 v) {
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
    return __builtin_bit_cast(u16x4, __builtin_convertvector(v, bf16x4));     // 2 x v_cvt_pk_bf16_f32
}

// explicitly global (address space 1) views: a pointer that went through an asm pin is no longer provably global,
// and hipcc would fall back to flat_ instructions
typedef __attribute__((address_space(1))) unsigned char gbyte;
typedef __attribute__((address_space(1))) u16x4 g_u16x4;
typedef __attribute__((address_space(1))) u16x8 g_u16x8;
__device__ __forceinline__ gbyte* to_global(const void* p) { return (gbyte*)(const_cast<void*>(p)); }
__device__ __forceinline__ void pins(gbyte*& p) { asm volatile("" : "+s"(p)); }
// a wave-uniform pointer the compiler has lost track of (state captured by a step lambda), back in scalar registers
template <typename T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<T*>(((unsigned long long)hi << 32) | lo);
}
// the data a pipelined stack hands over (saved h rows forward, gate gradients backward) leaves WRITE-THROUGH (common.h)
__device__ __forceinline__ void store16_wt(gbyte* uniform_base, unsigned lane_off, u16x8 v) {
    ::store16_wt((const void*)uniform_base, lane_off, v);
}

}  // namespace
