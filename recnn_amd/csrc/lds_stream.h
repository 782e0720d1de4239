// lds_stream.h -- the low-level idioms of the kernels that stream operands into LDS (gfx950): the LDS-DMA instruction in its two
// forms, counted vector-memory waits, transpose-read MFMA fragments, a one-dword read through the scalar cache and the shader-clock
// stamps of the in-kernel traces.  One definition each: a rule learned in one kernel (when M0 may be clobbered, why a form has no
// "memory" clobber, where a trace pointer must be computed) holds for every user.
#pragma once
#include "common.h"

// ---------------------------------------------------------------- LDS DMA and its waits
// One LDS-DMA instruction, saddr form: 64 lanes x 16 bytes from (uniform base + per-lane 32-bit byte offset) to LDS at lds_dst + 16 lane.
// The saddr form keeps a stage's address arithmetic to scalar adds.  M0 is written directly (the kernels that use it have no other
// M0 consumer: no movrel, no GWS, no LDS-direct loads); no "memory" clobber: the ordering points are the waits and barriers of the
// consumer, and the argument block stays in registers.
// clang warns that M0 is a reserved register on a clobber list.  The clobber is intended: it tells the compiler that M0 does not
// survive the statement; saving and restoring it, as dma16 does, would add two scalar moves to every DMA.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void dma_s(unsigned voff, const void* sbase, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(__builtin_amdgcn_readfirstlane(lds_dst)) : "m0");
}
#pragma clang diagnostic pop

// The same transfer from a per-lane flat address; M0 is saved and restored, so it is safe next to any other M0 consumer.
__device__ __forceinline__ void dma16(const void* gsrc, unsigned lds_dst_uniform) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_dst_uniform)
      : "memory");
}

// wait until at most N of this wave's vector-memory operations are outstanding (the asm DMAs are invisible to hipcc's wait insertion)
template <int N> __device__ __forceinline__ void wait_vm_const() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// ... with a run-time, wave-uniform n (0 .. 6; more waits for 6), and for every LDS / scalar operation as well
__device__ __forceinline__ void wait_vm(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory"); break;
  }
}

// ---------------------------------------------------------------- transpose-read fragments
typedef short v4s16 __attribute__((ext_vector_type(4)));   // what one ds_read_b64_tr_b16 returns
// two transpose reads = the 8 k values of a lane (k = 8 fg + 0..3 | 4..7): one bf16 MFMA operand
struct TrFrag {
  v4s16 lo, hi;
  __device__ __forceinline__ bf16x8 to_bf16x8() const { return __builtin_bit_cast(bf16x8, *this); }
};

// transpose-read fragment of 16 physical columns [col0, col0 + 16) over k rows 0..31 of an LDS image with `pitch` bytes per row
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* s, int pitch, int col0, int fr, int fg) {
  TrFrag f;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int row = fg * 8 + half * 4 + (fr >> 2);
    const v4s16 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) v4s16*)(s + row * pitch + (col0 + (fr & 3) * 4) * 2));
    if (half == 0) f.lo = v; else f.hi = v;
  }
  return f.to_bf16x8();
}

// The same fragment from a SWIZZLED image (pitch 256 bytes, no padding): the 32-byte chunk c of row r lives at chunk c ^ swz32(r).
// A transpose read's lane group touches rows {0..3, 8..11} (+4, +16) and 32 bytes of each: with a plain pitch of 256 + 16 (the x3 dW
// kernel's first layout) neighbouring rows overlap in 4 of their 8 banks -- a third of that kernel's LDS cycles were conflicts
// (SQ_LDS_BANK_CONFLICT, profiles/r04_x3_pmc.txt); swz32 maps the 8 rows to the 8 disjoint bank windows.
__device__ __forceinline__ int swz32(int row) { return (row & 3) | (((row >> 3) & 1) << 2); }
__device__ __forceinline__ bf16x8 tr_frag_swz(const unsigned char* s, int col0, int fr, int fg) {
  TrFrag f;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int row = fg * 8 + half * 4 + (fr >> 2);
    const v4s16 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) v4s16*)(s + row * 256 + (((col0 >> 4) ^ swz32(row)) << 5) + (fr & 3) * 8));
    if (half == 0) f.lo = v; else f.hi = v;
  }
  return f.to_bf16x8();
}

// ---------------------------------------------------------------- one dword through the scalar cache
// Requests *p into an SGPR and does NOT wait: the caller's first use of dst comes later (hipcc turns a plain load of a uniform global
// into a vector load + an immediate vmcnt(0), which drains every DMA in flight).  dst keeps its old value where the call is skipped.
__device__ __forceinline__ void sload_dword(int32_t& dst, const int32_t* p) { asm volatile("s_load_dword %0, %1, 0x0" : "=s"(dst) : "s"(p)); }
__device__ __forceinline__ void sload_dword(float& dst, const float* p) { asm volatile("s_load_dword %0, %1, 0x0" : "=s"(dst) : "s"(p)); }

// ---------------------------------------------------------------- in-kernel trace stamps (tools/*_trace.py)
// The stamp row of a workgroup: thread 0 of workgroup `wg` writes `slots` shader-clock stamps at trace + wg * slots; null in every
// other thread and when tracing is off.  The row pointer is computed ONCE, before any DMA is in flight, and pinned in a VGPR:
// gridDim.x is a load from the dispatch packet, and the compiler's vmcnt(0) for it inside a stamp drained the whole DMA queue of
// wave 0 at every stamp -- the first traces of mlps.hip charged that drain to whatever phase a stamp followed.
// (A macro: `wg` is evaluated inside the traced branch only, so an untraced launch never loads gridDim.)
#define TRACE_ROW(trace, wg, slots)                                                                                      \
  ({                                                                                                                     \
    unsigned long long* row_ = ((trace) && threadIdx.x == 0) ? (trace) + (int64_t)(wg) * (slots) : nullptr;              \
    asm volatile("" : "+v"(row_));                                                                                       \
    row_;                                                                                                                \
  })
#define TRACE_STAMP(trow, i) do { if (trow) (trow)[(i)] = __builtin_amdgcn_s_memtime(); } while (0)
