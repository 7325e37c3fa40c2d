// TEST INFRASTRUCTURE: what tests/c/hip_stub_rtc_fb.cpp logs, for tests/c/engine_host_driver_dk_fb.cpp.
#pragma once
#include <string>
#include <vector>

#include "../../rocoder_amd/csrc/rc_rtc.h"

struct RtcFbLaunch {
    int pass;  // 0: rc_user_dk, 1: rc_user_dk_sums_pass
    unsigned gx, gy, gz, bx;
    const void *stream;
    rc::UserDkArgs a;    // the argument block as the launch carried it
    size_t state_bytes;  // the size of the allocation that starts at a.state (0: none starts there, or no state)
};
// the launches / the hipModuleGetFunction names since the last call, in order
std::vector<RtcFbLaunch> rtc_fb_stub_take_launches();
std::vector<std::string> rtc_fb_stub_take_lookups();
