// pt_step_addr.h — when the fused step kernel (k_wf_step_bf, pt_wf_bf.hip) may address a part's
// queues with 32-bit byte offsets.  A rule for the host, in standard C++ (constexpr only, so it also
// compiles into the device units that include pt_kernels.h; scripts/step_addr_harness.cpp checks the
// boundary on the CPU).
//
// The 32-bit instances reach an array as a wave-uniform 64-bit base (SGPRs) plus a per-lane 32-bit
// byte offset (global_load/store v_off, s[base:base+1]): no 64-bit VALU per access.  The widest
// arrays by byte offset are `ray` (two float4, 32 B per entry; q2, q3, sp0 take 16 B, sp2 8 B) over
// the part's qcap entries, and `rad` (three floats, 12 B per path) over the part's paths.  An offset
// fits while the array's extent in bytes does; a part beyond that is launched with the 64-bit
// instances (the same kernel body, kStepAddr64), never narrowed.
#pragma once
#include <cstdint>

namespace pt {

constexpr uint64_t kStepRayEntryBytes = 32;  // WfQueue::ray: 2 x float4 per entry
constexpr uint64_t kStepRadPathBytes = 12;   // WfBuffers::rad: 3 x float per path

// qcap: entries per queue array of the part; paths: the part's paths (its radiance)
constexpr bool step_addr32_ok(uint64_t qcap, uint64_t paths) {
    // (as quotients: no product to wrap, whatever the caller passes)
    return qcap <= 0xffffffffull / kStepRayEntryBytes && paths <= 0xffffffffull / kStepRadPathBytes;
}

}  // namespace pt
