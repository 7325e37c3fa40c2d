// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The launchers of rocoder_amd/csrc/rc_long.hip for the host-only engine builds (tests/c/hip_stub.cpp has the rest):
// they compute nothing, as every stubbed launcher.
#include <hip/hip_runtime_api.h>

#include "../../rocoder_amd/csrc/rc_long.h"

namespace rc {
hipError_t launch_long(int, const LongParams &, hipStream_t) { return hipSuccess; }
hipError_t launch_long_ola(const OlaParams &, hipStream_t, bool) { return hipSuccess; }
}  // namespace rc
