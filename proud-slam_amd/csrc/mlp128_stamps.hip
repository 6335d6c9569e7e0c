// Diagnostic build only (`make stamps`, -DPSVO_STAMPS: lib/diag/, never the
// product library): the width-128 decoder's files as one translation unit,
// in place of their objects — their kernels write one __device__ stamp array
// (mlp128.h) and the build has no relocatable device code.
#ifndef PSVO_STAMPS
#error "mlp128_stamps.hip is the -DPSVO_STAMPS build of the width-128 decoder"
#endif
#include "mlp_fwd.hip"
#include "mlp_bwd.hip"

// copies the stamp array ([3 kernels][256 wg][8 waves][8 tiles][16 points] u64)
extern "C" int psvo_debug_stamps(void *dst, int64_t bytes) {
    if (bytes < (int64_t)sizeof(psvo_g_stamps)) return -1;
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(psvo_g_stamps), sizeof(psvo_g_stamps)) == hipSuccess ? 0 : -2;
}
