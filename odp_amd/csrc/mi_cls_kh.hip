// mi_cls_kh.hip -- the transmit kernel's instantiations with the pktin flow
// hash (mi_cls_tx_kernel<TX_M_CK_HASH> / <TX_M_HASH>, mi_cls_tx_dev.h) and
// their launcher.
#include "mi_cls_tx_dev.h"

int mi_cls_launch_tx_hash(bool ck, unsigned grid, hipStream_t st, const TxHashArgs &a)
{
#ifdef MI_CLS_STUB
	(void)ck;
	(void)grid;
	(void)st;
	(void)a;
	return -ENOSYS;
#else
	const void *k = ck ? reinterpret_cast<const void *>(&mi_cls_tx_kernel<TX_M_CK_HASH, TxHashArgs>)
			   : reinterpret_cast<const void *>(&mi_cls_tx_kernel<TX_M_HASH, TxHashArgs>);
	if (grid == 0) {   // preload (mi_cls_ctx_create)
		hipFuncAttributes fa;
		return hipFuncGetAttributes(&fa, k) == hipSuccess ? 0 : -EIO;
	}
	void *args[] = { (void *)&a };
	return hipLaunchKernel(k, dim3(grid), dim3(TX_NW * WAVE), args, 0, st) == hipSuccess ? 0 : -EIO;
#endif
}
