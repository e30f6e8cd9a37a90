// BN-256 twist (F_p^2): the bucket stage and the recombination of several scalar rows over one table
#include "bn256_impl.h"

template int bn_kernels<G2, BnF2>::bucket_rows(vmpc_ctx *, const msm_plan &, const msm_ws *, int, const uint32_t *);
template int bn_kernels<G2, BnF2>::final_rows(vmpc_ctx *, const msm_plan &, msm_ws &, void *, int);
