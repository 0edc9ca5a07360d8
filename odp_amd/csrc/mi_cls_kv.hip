// mi_cls_kv.hip -- the vector fill's kernels (mi_cls_vec_dev.h) and their
// launcher: count, place, fill and the counters' hand-over are launches of
// their own on the stream.
#include "mi_cls_vec_dev.h"

#ifndef MI_CLS_STUB
static int vec_launch(const void *k, unsigned grid, unsigned block, hipStream_t st, const VecArgs &a, bool preload)
{
	if (preload) {
		hipFuncAttributes fa;
		return hipFuncGetAttributes(&fa, k) == hipSuccess ? 0 : -EIO;
	}
	void *args[] = { (void *)&a };
	return hipLaunchKernel(k, dim3(grid), dim3(block), args, 0, st) == hipSuccess ? 0 : -EIO;
}
#endif

int mi_cls_launch_vec(hipStream_t st, const VecArgs &a, bool preload)
{
#ifdef MI_CLS_STUB
	(void)st;
	(void)a;
	(void)preload;
	return -ENOSYS;
#else
	const void *count = reinterpret_cast<const void *>(&mi_cls_vec_count_kernel);
	const void *place = reinterpret_cast<const void *>(&mi_cls_vec_place_kernel);
	const void *fill = reinterpret_cast<const void *>(&mi_cls_vec_fill_kernel);
	const void *finish = reinterpret_cast<const void *>(&mi_cls_vec_finish_kernel);
	int rc = 0;
	if (preload || a.n) {
		rc = vec_launch(count, a.grid, VEC_THREADS, st, a, preload);
		if (!rc)
			rc = vec_launch(place, a.grid, VEC_THREADS, st, a, preload);
		if (!rc)
			rc = vec_launch(fill, a.fgrid, VEC_THREADS, st, a, preload);
	}
	if (!rc)
		rc = vec_launch(finish, 1, VEC_THREADS, st, a, preload);
	return rc;
#endif
}
