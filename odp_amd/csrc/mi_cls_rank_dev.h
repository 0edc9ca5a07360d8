// mi_cls_rank_dev.h -- the wave step of a stable rank, shared by the receive
// chain's decide kernel (mi_cls_kd.hip), the enqueue plan's kernels
// (mi_cls_enq_dev.h) and the pool plan's (mi_cls_pool_dev.h): a lane's rank
// among the lanes of its value is
// popcount(match_lanes(v) & lanes below); the counts of the waves before it
// are the caller's.
#ifndef MI_CLS_RANK_DEV_H_
#define MI_CLS_RANK_DEV_H_

#include "mi_cls_dev.h"

// The lanes of the wave whose value equals this lane's (values below 2^bits):
// one ballot per bit, no loop over the distinct values.
__device__ __forceinline__ unsigned long long match_lanes(uint32_t v, int bits)
{
	unsigned long long m = ~0ull;
	for (int b = 0; b < bits; ++b) {
		const bool x = ((v >> b) & 1u) != 0u;
		const unsigned long long bb = __ballot(x);
		m &= x ? bb : ~bb;
	}
	return m;
}

#endif /* MI_CLS_RANK_DEV_H_ */
