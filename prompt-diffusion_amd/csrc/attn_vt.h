// The key order of a 2-byte V^T tile in LDS, shared by attention.hip and vae_attention.hip.
#pragma once
#include "pd_common.h"

// The S^T accumulator of a 16-key tile holds keys 4*fq + j for lane quarter fq.  The 8 keys one lane feeds to a K = 32 PV MFMA are
// keys 4*fq + j of the two 16-key S^T tiles 2u and 2u+1 -- the order P already has in registers -- so a V^T row holds its keys PERMUTED
// inside each group of 32 to make those 8 keys 16 contiguous bytes:
//   slot(key) = 32*(key/32) + 8*((key%16)/4) + 4*((key%32)/16) + key%4        (a 2-byte element index inside the row)
__device__ __forceinline__ int vt_slot(int k0) { return (k0 & ~31) + (((k0 & 15) >> 2) << 3) + (((k0 & 31) >> 4) << 2); }
