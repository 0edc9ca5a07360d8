// mi_cls_kr.hip -- the run plan's kernels (mi_cls_run_dev.h) and their
// launcher: every step of the plan is a launch of its own on the stream.
#include "mi_cls_run_dev.h"

#ifndef MI_CLS_STUB
static int run_launch(const void *k, unsigned grid, unsigned block, hipStream_t st, const RunArgs &a, bool preload)
{
	if (preload) {
		hipFuncAttributes fa;
		return hipFuncGetAttributes(&fa, k) == hipSuccess ? 0 : -EIO;
	}
	void *args[] = { (void *)&a };
	return hipLaunchKernel(k, dim3(grid), dim3(block), args, 0, st) == hipSuccess ? 0 : -EIO;
}
#endif

int mi_cls_launch_run(hipStream_t st, const RunArgs &a, bool preload)
{
#ifdef MI_CLS_STUB
	(void)st;
	(void)a;
	(void)preload;
	return -ENOSYS;
#else
	const void *key = reinterpret_cast<const void *>(&mi_cls_run_key_kernel);
	const void *scan = reinterpret_cast<const void *>(&mi_cls_run_scan_kernel);
	const void *scatter = reinterpret_cast<const void *>(&mi_cls_run_scatter_kernel);
	const void *finish = reinterpret_cast<const void *>(&mi_cls_run_finish_kernel);
	const void *out = reinterpret_cast<const void *>(&mi_cls_run_out_kernel);
	int rc = 0;
	auto run = [&](const void *k, unsigned grid, unsigned block) {
		if (!rc)
			rc = run_launch(k, grid, block, st, a, preload);
	};
	if (preload || a.n) {
		run(key, a.grid, RUN_THREADS);
		run(scan, 1, MI_CLS_RUN_GRID);
		run(scatter, a.grid, RUN_THREADS);
		// thread r of 0 .. nruns (<= n, known to the device alone): the key
		// launch's grid (one block per tile), then grid-stride
		run(finish, a.grid, RUN_FIN_THREADS);
	}
	run(out, 1, WAVE);
	return rc;
#endif
}
