// mi_cls_ka.hip -- the pool plan's kernels (mi_cls_pool_dev.h) and their
// launcher: every step of the plan is a launch of its own on the stream.
#include "mi_cls_pool_dev.h"

#ifndef MI_CLS_STUB
static int pool_launch(const void *k, unsigned grid, hipStream_t st, const PoolArgs &a, bool preload)
{
	if (preload) {
		hipFuncAttributes fa;
		return hipFuncGetAttributes(&fa, k) == hipSuccess ? 0 : -EIO;
	}
	void *args[] = { (void *)&a };
	return hipLaunchKernel(k, dim3(grid), dim3(POOL_THREADS), args, 0, st) == hipSuccess ? 0 : -EIO;
}
#endif

int mi_cls_launch_pool(hipStream_t st, const PoolArgs &a, bool preload)
{
#ifdef MI_CLS_STUB
	(void)st;
	(void)a;
	(void)preload;
	return -ENOSYS;
#else
	const void *count = reinterpret_cast<const void *>(&mi_cls_pool_count_kernel);
	const void *place = reinterpret_cast<const void *>(&mi_cls_pool_place_kernel);
	const void *finish = reinterpret_cast<const void *>(&mi_cls_pool_finish_kernel);
	int rc = 0;
	if (preload || a.n) {
		rc = pool_launch(count, a.grid, st, a, preload);
		if (!rc)
			rc = pool_launch(place, a.grid, st, a, preload);
	}
	if (!rc)
		rc = pool_launch(finish, 1, st, a, preload);
	return rc;
#endif
}
