// ADMP_* environment switches (README.md has the table): the one place that parses them.  Host only.
#pragma once
#include <cstdlib>

inline int env_int(const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; }
// set to 0: false; set to anything else: true; unset: dflt
inline bool env_flag(const char* name, bool dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) != 0 : dflt; }
