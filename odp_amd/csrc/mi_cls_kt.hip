// mi_cls_kt.hip -- the pktout checksum insertion kernel (mi_cls_tx_kernel,
// mi_cls_tx_dev.h) and its launcher.
#include "mi_cls_tx_dev.h"

int mi_cls_launch_tx(unsigned grid, hipStream_t st, const TxArgs &a)
{
#ifdef MI_CLS_STUB
	(void)grid;
	(void)st;
	(void)a;
	return -ENOSYS;
#else
	if (grid == 0) {   // preload (mi_cls_ctx_create)
		hipFuncAttributes fa;
		return hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&mi_cls_tx_kernel<TX_M_CK, TxArgs>)) ==
		       hipSuccess ? 0 : -EIO;
	}
	void *args[] = { (void *)&a };
	return hipLaunchKernel(reinterpret_cast<const void *>(&mi_cls_tx_kernel<TX_M_CK, TxArgs>), dim3(grid),
			       dim3(TX_NW * WAVE), args, 0, st) == hipSuccess ? 0 : -EIO;
#endif
}
