// mi_cls_kq.hip -- the enqueue plan's kernels (mi_cls_enq_dev.h) and their
// launcher: every step of the plan is a launch of its own on the stream.
#include "mi_cls_enq_dev.h"

#ifndef MI_CLS_STUB
static int enq_launch(const void *k, unsigned grid, unsigned block, hipStream_t st, const EnqArgs &a, bool preload)
{
	if (preload) {
		hipFuncAttributes fa;
		return hipFuncGetAttributes(&fa, k) == hipSuccess ? 0 : -EIO;
	}
	void *args[] = { (void *)&a };
	return hipLaunchKernel(k, dim3(grid), dim3(block), args, 0, st) == hipSuccess ? 0 : -EIO;
}
#endif

int mi_cls_launch_enq(hipStream_t st, const EnqArgs &a, int passes, bool preload)
{
#ifdef MI_CLS_STUB
	(void)st;
	(void)a;
	(void)passes;
	(void)preload;
	return -ENOSYS;
#else
	const void *key = reinterpret_cast<const void *>(&mi_cls_enq_key_kernel);
	const void *scan = reinterpret_cast<const void *>(&mi_cls_enq_scan_kernel);
	const void *count = reinterpret_cast<const void *>(&mi_cls_enq_count_kernel);
	const void *one = reinterpret_cast<const void *>(&mi_cls_enq_scatter_kernel<0, true>);
	const void *low = reinterpret_cast<const void *>(&mi_cls_enq_scatter_kernel<0, false>);
	const void *high = reinterpret_cast<const void *>(&mi_cls_enq_scatter_kernel<1, true>);
	const void *gbeg = reinterpret_cast<const void *>(&mi_cls_enq_gbeg_kernel);
	int rc = 0;
	auto run = [&](const void *k, unsigned grid, unsigned block) {
		if (!rc)
			rc = enq_launch(k, grid, block, st, a, preload);
	};
	if (preload || a.n) {
		run(key, a.grid, ENQ_THREADS);
		run(scan, 1, ENQ_THREADS);
		if (preload || passes == 1)
			run(one, a.grid, ENQ_THREADS);
		if (preload || passes != 1) {
			run(low, a.grid, ENQ_THREADS);
			run(count, a.grid, ENQ_THREADS);
			run(scan, 1, ENQ_THREADS);
			run(high, a.grid, ENQ_THREADS);
		}
	}
	// thread j of 0 .. n (one pass: thread g of 0 .. ndst + 1); at most 1024
	// blocks, then grid-stride
	const unsigned long long gb = ((passes == 1 ? a.ndst + 1ull : (unsigned long long)a.n) + ENQ_GB_THREADS) /
				      ENQ_GB_THREADS;
	run(gbeg, (unsigned)(gb < 1024ull ? gb : 1024ull), ENQ_GB_THREADS);
	return rc;
#endif
}
