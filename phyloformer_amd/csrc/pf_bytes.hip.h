// Byte runs at any address, shared by the gathers that build derived alignments (pf_sites.hip.h, pf_taxa.hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfbytes {

// four contiguous source bytes at any address, as the little-endian dword a 4-byte store writes
__device__ inline uint32_t load_run4(const uint8_t* p) {
    const uintptr_t ad = reinterpret_cast<uintptr_t>(p);
    if ((ad & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
    if ((ad & 1) == 0)
        return (uint32_t)*reinterpret_cast<const uint16_t*>(p) | ((uint32_t)*reinterpret_cast<const uint16_t*>(p + 2) << 16);
    return (uint32_t)p[0] | ((uint32_t)*reinterpret_cast<const uint16_t*>(p + 1) << 8) | ((uint32_t)p[3] << 24);
}

}  // namespace pfbytes
