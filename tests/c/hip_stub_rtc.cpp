// TEST INFRASTRUCTURE (host sanitizer builds only; never linked into the product library).
// The HIP module calls of rocoder_amd/csrc/rc_rtc.cpp for the host-only engine builds (tests/c/hip_stub.cpp has the
// rest): a module is a host allocation, its kernel computes nothing, every event has completed.
#include <hip/hip_runtime_api.h>

#include <cstdlib>

extern "C" {
hipError_t hipModuleLoadData(hipModule_t *m, const void *) {
    *m = (hipModule_t)malloc(16);
    return *m ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipModuleUnload(hipModule_t m) {
    free((void *)m);
    return hipSuccess;
}
hipError_t hipModuleGetFunction(hipFunction_t *f, hipModule_t m, const char *) {
    *f = (hipFunction_t)m;
    return hipSuccess;
}
hipError_t hipModuleLaunchKernel(hipFunction_t, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned,
                                 hipStream_t, void **, void **) {
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
}
