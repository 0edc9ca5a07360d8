// mi_cls_kl.hip -- the LSO segmentation kernel (mi_cls_lso_kernel,
// mi_cls_lso_dev.h) and its launcher.
#include "mi_cls_lso_dev.h"

int mi_cls_launch_lso(unsigned grid, hipStream_t st, const LsoArgs &a)
{
#ifdef MI_CLS_STUB
	(void)grid;
	(void)st;
	(void)a;
	return -ENOSYS;
#else
	if (grid == 0) {   // preload (mi_cls_ctx_create)
		hipFuncAttributes fa;
		return hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&mi_cls_lso_kernel)) ==
		       hipSuccess ? 0 : -EIO;
	}
	void *args[] = { (void *)&a };
	return hipLaunchKernel(reinterpret_cast<const void *>(&mi_cls_lso_kernel), dim3(grid),
			       dim3(LSO_NW * WAVE), args, 0, st) == hipSuccess ? 0 : -EIO;
#endif
}
