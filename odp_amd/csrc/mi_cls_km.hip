// mi_cls_km.hip -- the pool move's kernels (mi_cls_move_dev.h) and their
// launcher: the move and the counters' hand-over are launches of their own on
// the stream.
#include "mi_cls_move_dev.h"

#ifndef MI_CLS_STUB
static int move_launch(const void *k, unsigned grid, unsigned block, hipStream_t st, const MoveArgs &a, bool preload)
{
	if (preload) {
		hipFuncAttributes fa;
		return hipFuncGetAttributes(&fa, k) == hipSuccess ? 0 : -EIO;
	}
	void *args[] = { (void *)&a };
	return hipLaunchKernel(k, dim3(grid), dim3(block), args, 0, st) == hipSuccess ? 0 : -EIO;
}
#endif

int mi_cls_launch_move(hipStream_t st, const MoveArgs &a, bool preload)
{
#ifdef MI_CLS_STUB
	(void)st;
	(void)a;
	(void)preload;
	return -ENOSYS;
#else
	const void *move = reinterpret_cast<const void *>(&mi_cls_move_kernel<false>);
	const void *move_pk = reinterpret_cast<const void *>(&mi_cls_move_kernel<true>);
	const void *finish = reinterpret_cast<const void *>(&mi_cls_move_finish_kernel);
	int rc = 0;
	if (preload)
		rc = move_launch(move, 0, MOVE_THREADS, st, a, true);
	if (!rc && (preload || a.n))
		rc = move_launch(a.pk || preload ? move_pk : move, a.grid, MOVE_THREADS, st, a, preload);
	if (!rc)
		rc = move_launch(finish, 1, WAVE, st, a, preload);
	return rc;
#endif
}
