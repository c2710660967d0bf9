// The head generator of the pruned selection's bound pass under a short residue plan (kgen_kernel<FAM, DP, 10, true>: the columns
// k < res_kmax alone, 10 residue planes at the short plan's scale res_sK).  Core and design notes: kgen_core.h, kgen.hip.
#include "kgen_core.h"

namespace abo {

hipError_t launch_kgen_res_short10(const KgenArgs& a, hipStream_t s) { return launch_kgen_res_short<10>(a, s); }

}  // namespace abo
