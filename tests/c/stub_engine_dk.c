/* TEST INFRASTRUCTURE - never shipped, never linked into the product. The user-device-kernel entry points of the stub
 * engine (tests/c/stub_engine.c) for the ThreadSanitizer build of the CLI: rc_dk_compile "compiles" any source that
 * names rc_apply into a few bytes, so the --device-kernel-src watcher thread and the hand-over to the thread that
 * drives the engine run without hiprtc or a GPU. */
#include <string.h>

#include "rocoder_hip.h"

int rc_dk_compile(const char *src, size_t src_len, char *code, size_t code_cap, size_t *code_len, char *log,
                  size_t log_cap) {
    static const char obj[] = "stub code object";
    size_t i;
    int found = 0;
    if (log && log_cap) log[0] = 0;
    if (!src || !code_len) return RC_EINVAL;
    *code_len = sizeof obj;
    for (i = 0; i + 8 <= src_len && !found; ++i) found = memcmp(src + i, "rc_apply", 8) == 0;
    if (!found) {
        if (log && log_cap) strncpy(log, "stub: no rc_apply", log_cap - 1), log[log_cap - 1] = 0;
        return RC_EINVAL;
    }
    if (!code || code_cap < sizeof obj) return RC_ECAPACITY;
    memcpy(code, obj, sizeof obj);
    return RC_OK;
}
int rc_engine_load_device_kernel(rc_engine *e, const char *code, size_t code_len) {
    (void)code; (void)code_len;
    return e ? RC_OK : RC_EINVAL;
}
int rc_engine_set_device_kernel_params(rc_engine *e, const float *params, uint32_t n_params) {
    (void)params;
    return e && n_params <= 16 ? RC_OK : RC_EINVAL;
}
int rc_multi_load_device_kernel(rc_multi *m, const char *code, size_t code_len) {
    (void)m; (void)code; (void)code_len;
    return RC_EUNSUPPORTED;
}
int rc_multi_set_device_kernel_params(rc_multi *m, const float *params, uint32_t n_params) {
    (void)m; (void)params; (void)n_params;
    return RC_EUNSUPPORTED;
}
