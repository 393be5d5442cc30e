// The PGF_* environment switches (host).  gfx950 (MI355X / CDNA4) only.
#pragma once

#include <cstdlib>

// The PGF_* environment switches (host).  Each call site keeps its value in a `static const', so a
// variable is read once per process, the first time its code path runs.
inline bool env_on(const char *name) {  // on unless set to 0
  const char *e = getenv(name);
  return !(e && atoi(e) == 0);
}
inline int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline double env_double(const char *name, double dflt) {
  const char *e = getenv(name);
  return e ? atof(e) : dflt;
}
