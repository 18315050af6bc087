// The one reader of the SKIMI_* environment switches that pick a kernel or a model variant (host only, plain C++).
//   env_once(name, dflt)    read at the first call for that name, kept for the life of the process
//   env_switch(name, dflt)  the same, but under SKIMI_ENV_DYNAMIC=1 (itself read once) read again on every call:
//                           in-process A/B timing (tools/ab_*.py) and the tests' variant sweeps
// Unset gives dflt; a set value is parsed by atol ("0" and text that is no number give 0); a site that used atoi
// converts to int, which truncates as atoi does.  The few switches read on every call whatever SKIMI_ENV_DYNAMIC
// says (model build, profiling builds) stay a plain getenv at their site.
#pragma once
#include <stdlib.h>

#include <map>
#include <mutex>
#include <string>
#include <string_view>

namespace skimi {

inline long env_read(const char* name, long dflt) {
    const char* v = getenv(name);
    return v ? atol(v) : dflt;
}

inline long env_once(const char* name, long dflt) {
    static std::mutex mu;
    static std::map<std::string, long, std::less<>> seen;
    std::lock_guard<std::mutex> lock(mu);
    const auto it = seen.find(std::string_view(name));
    if (it != seen.end()) return it->second;
    return seen.emplace(name, env_read(name, dflt)).first->second;
}

inline long env_switch(const char* name, long dflt) {
    static const bool dynamic = [] {
        const char* v = getenv("SKIMI_ENV_DYNAMIC");
        return v && atoi(v);
    }();
    return dynamic ? env_read(name, dflt) : env_once(name, dflt);
}

}  // namespace skimi
