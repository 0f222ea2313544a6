// The tagged-granule hand-off, device side: the one place the protocol of the
// direct xGMI halo exchange (stage_kernel.hip, march_kernel.hip, fused_step.hip)
// and of the fused step's in-launch hand-off buffer lives.
//
// Tagged granules: the data is the flag.  A record (the field values of one
// ghost cell) travels as W 8-byte granules {tag, payload} (codecs: xg_codec.h),
// each one relaxed atomic store.  An aligned 8-byte access is single-copy
// atomic, so a granule is never torn: a reader sees the old granule or the new
// one.  The consumer thread re-reads its record's granules until every tag is
// the one it waits for.  The producer neither drains nor signals and the
// consumer makes no separate poll round trip (cdna_hip_programming.md
// Guideline 16, R2).  The wait is bounded: a timeout, or an `err` word another
// waiter has already set, ends it, and the caller records the failure.
//
// Tags only grow.  Epoch e (a per-block count of completed stages / steps)
// reads its input records under tag e + 1 and writes its output under tag
// e + 2, the input tag of epoch e + 1.  Nothing is ever reset.
//
// Ring slots.  A rank reads slot e % S during its stage e while a peer writes
// slot (e_p + 1) % S during its stage e_p.  A peer can have STARTED at most two
// stages past us: its stage e + 2 needs its stage e + 1 complete, which waited
// for our stage-e output, i.e. our stage e started and e - 1 completed.  So the
// peer writes slot (e + 1 .. e + 3) % S, never e % S, iff S does not divide 1,
// 2 or 3: S = 4 (three slots left a window where a peer two stages ahead
// overwrote the slot a slow block of ours was still reading).  A slot thus
// holds the record waited for or the one S stages older; the packed codec's
// 12-bit tag window (xg_codec.h) relies on that.
//
// Record layout.  A ring slot holds `ring` granules = nrec records of W words,
// word-major: word w of record r at w nrec + r.  The host numbers a consumer's
// records by owner rank, then cell id (row order), so the lanes of one store or
// poll instruction touch consecutive 8-byte words (up to 512 contiguous bytes
// per wave).  The fused step's hand-off buffer is addressed the same way
// (base + k stride, stride = cells per slot).
#pragma once
#include "xg_codec.h"

#define STSP_XG_SLOTS 4

namespace {

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned int gu32;

// memory scope of the granule accesses: a ring is written by other GPUs, the
// fused step's hand-off buffer only by other workgroups of the same launch
constexpr int XG_RING_SCOPE = __HIP_MEMORY_SCOPE_SYSTEM;
constexpr int XG_LOCAL_SCOPE = __HIP_MEMORY_SCOPE_AGENT;

// slot and tag arithmetic of epoch e
__device__ __forceinline__ int xg_in_slot(int e) { return e % STSP_XG_SLOTS; }
__device__ __forceinline__ int xg_out_slot(int e) { return (e + 1) % STSP_XG_SLOTS; }
__device__ __forceinline__ unsigned xg_in_tag(int e) { return (unsigned)e + 1u; }
__device__ __forceinline__ unsigned xg_out_tag(int e) { return (unsigned)e + 2u; }

// first granule of a record and the distance between its granules
struct XgRec {
  gu64* p;
  long stride;
};

// record `rec` of slot `slot` of the ring at `base` (`ring` granules per slot)
template <class C>
__device__ __forceinline__ XgRec ring_slot_record(const void* base, int ring, int slot, int rec) {
  return {(gu64*)base + (long)slot * ring + rec, (long)(ring / C::W)};
}
// the record a push code (peer << 24 | record) names, in that peer's ring
template <class C, typename P>
__device__ __forceinline__ XgRec ring_record(P* const* peer_ring, int ring, int code, int slot) {
  return ring_slot_record<C>(peer_ring[code >> 24], ring, slot, code & 0xFFFFFF);
}

template <class C, int SCOPE>
__device__ __forceinline__ void xg_store(XgRec r, const unsigned long long (&g)[C::W]) {
#pragma unroll
  for (int k = 0; k < C::W; ++k) __hip_atomic_store(r.p + k * r.stride, g[k], __ATOMIC_RELAXED, SCOPE);
}

// Initial delivery (prime kernels): cell `src` of the state q (F fields, stride
// S) as an input record of epoch `epoch`, into the ring `code` names.
template <class C, int F, typename T>
__device__ __forceinline__ void xg_prime_record(const T* q, int S, int src, int code, T* const* peer_ring, int ring,
                                                int epoch) {
  T v[F];
#pragma unroll
  for (int f = 0; f < F; ++f) v[f] = q[(long)f * S + src];
  unsigned long long g[C::W];
  C::pack(v, xg_in_tag(epoch), g);
  xg_store<C, XG_RING_SCOPE>(ring_record<C>(peer_ring, ring, code, xg_in_slot(epoch)), g);
}

enum class XgWait { ok, aborted, timeout };   // aborted: err was already set

// The bounded spin of every in-kernel wait: poll `arrived()` until it holds,
// `err` is set or the timeout passes.  The error word is read only after a
// poll that failed, so what has already arrived (the common case) costs no
// error-word traffic.  A timeout calls `on_timeout()`, the caller's record of
// the failure, inside the loop (recorded after it, the XG stage kernels'
// register allocation changes; profiles/xg_ring).  FENCE: the xgfence
// diagnostic (an acquire fence in front of every poll).
template <bool FENCE = false, class Poll, class Fail>
__device__ __forceinline__ XgWait xg_spin(const int* err, long long timeout_ticks, Poll arrived, Fail on_timeout) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  XgWait w = XgWait::ok;
  for (;;) {
    if (FENCE) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    if (arrived()) break;
    if (__hip_atomic_load((gu32*)err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) { w = XgWait::aborted; break; }
    if ((long long)(__builtin_amdgcn_s_memrealtime() - t0) > timeout_ticks) {
      on_timeout();
      w = XgWait::timeout;
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  return w;
}

// Re-read the record's granules into g until every tag is `want`.
template <class C, int SCOPE, bool FENCE = false, class Fail>
__device__ __forceinline__ XgWait xg_wait(XgRec r, unsigned want, const int* err, long long timeout_ticks,
                                          unsigned long long (&g)[C::W], Fail on_timeout) {
  return xg_spin<FENCE>(err, timeout_ticks, [&] {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < C::W; ++k) g[k] = __hip_atomic_load(r.p + k * r.stride, __ATOMIC_RELAXED, SCOPE);
#pragma unroll
    for (int k = 0; k < C::W; ++k) ok &= C::tag_ok(g[k], want);
    return ok;
  }, on_timeout);
}

}  // namespace
