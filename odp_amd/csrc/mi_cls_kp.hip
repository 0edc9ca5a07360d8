// mi_cls_kp.hip -- the parse-only kernel (mi_cls_parse_kernel,
// mi_cls_parse_dev.h) and its launcher: one instantiation per start protocol,
// with and without the checksum code.
#include "mi_cls_parse_dev.h"

#ifndef MI_CLS_STUB
template <uint32_t START, bool CK>
static int parse_launch(unsigned grid, hipStream_t st, const ParseArgs &a)
{
	const void *k = reinterpret_cast<const void *>(&mi_cls_parse_kernel<START, CK>);
	if (grid == 0) {   // preload (mi_cls_ctx_create)
		hipFuncAttributes fa;
		return hipFuncGetAttributes(&fa, k) == hipSuccess ? 0 : -EIO;
	}
	void *args[] = { (void *)&a };
	return hipLaunchKernel(k, dim3(grid), dim3(PRS_NW * WAVE), args, 0, st) == hipSuccess ? 0 : -EIO;
}
#endif

int mi_cls_launch_parse(uint32_t proto, bool ck, unsigned grid, hipStream_t st, const ParseArgs &a)
{
#ifdef MI_CLS_STUB
	(void)proto;
	(void)ck;
	(void)grid;
	(void)st;
	(void)a;
	return -ENOSYS;
#else
	switch (proto) {
	case MI_CLS_PROTO_ETH:
		return ck ? parse_launch<MI_CLS_PROTO_ETH, true>(grid, st, a)
			  : parse_launch<MI_CLS_PROTO_ETH, false>(grid, st, a);
	case MI_CLS_PROTO_IPV4:
		return ck ? parse_launch<MI_CLS_PROTO_IPV4, true>(grid, st, a)
			  : parse_launch<MI_CLS_PROTO_IPV4, false>(grid, st, a);
	case MI_CLS_PROTO_IPV6:
		return ck ? parse_launch<MI_CLS_PROTO_IPV6, true>(grid, st, a)
			  : parse_launch<MI_CLS_PROTO_IPV6, false>(grid, st, a);
	default:
		return -EINVAL;
	}
#endif
}
