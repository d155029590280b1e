// libbsms_hip_query.so (include/bsms_hip_query.h): the record plan_fwd / plan_bwd (chain_launch.h, in libbsms_hip.so) make for a key, as
// integers and a name.  Host code only.
#include "../chain.h"

extern "C" int bsms_chain_launch_query(int D, int backward, int mode_a, int mode_b, const bsms_chain_launch_key* key, int cus,
                                       bsms_chain_launch_info* out) {
  using namespace bsms;
  BSMS_REQUIRE(key != nullptr && out != nullptr, BSMS_E_INVALID_ARG, "chain_launch_query: null argument");
  BSMS_REQUIRE(key->R >= 1 && cus >= 0 && key->nstage >= 0 && key->nstage <= kMaxStages && key->nseq >= 0 && key->nseq <= kMaxStages + 2,
               BSMS_E_INVALID_ARG, "chain_launch_query: R=%lld cus=%d nstage=%d nseq=%d", (long long)key->R, cus, key->nstage, key->nseq);
  ChainLaunch l{};
  const int rc = with_width(D, [&](auto nb) {
    return chain_launch_query_nb<decltype(nb)::value>(backward, mode_a, mode_b, *key, cus ? cus : device_cu_count(), &l);
  });
  if (rc) return rc;
  *out = {l.family, l.rb, l.save, l.store, l.lone, l.bf16, l.timing, l.cw, l.nload, l.nring, l.ntiles, l.grid, l.threads, int64_t(l.lds), int64_t(l.lds_max), {}};
  const char* fam = l.family == CHAIN_FS ? (backward ? "fs_bwd" : "fs_fwd") : l.what;
  snprintf(out->name, sizeof out->name, "%s%s%s%s%s%s%s", fam, l.rb == 2 ? " rb2" : l.rb == 1 ? " rb1" : "", l.save ? " save" : "", l.store ? " store" : "",
           l.bf16 ? " bf16" : "", l.timing ? " timing" : "", l.lone ? " lone" : "");
  return BSMS_OK;
}
