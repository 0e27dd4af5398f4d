// The environment switches' table (env.h): parse rules, the snapshot, reload.
#include "env.h"

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace {
// The parse rules: v is the variable's text, never empty and shorter than 64
// characters (anything else is "unset" and takes the row's default).
int32_t parse_digit_0_to_4(const char* v, int32_t dflt) {
  return v[0] >= '0' && v[0] <= '4' ? v[0] - '0' : dflt;
}
int32_t parse_integer(const char* v, int32_t) { return (int32_t)strtol(v, nullptr, 10); }
uint32_t parse_unsigned_integer(const char* v, uint32_t) {
  return (uint32_t)strtoul(v, nullptr, 10);
}
bool parse_on_unless_0(const char* v, bool) { return v[0] != '0'; }
bool parse_on_if_1(const char* v, bool) { return v[0] == '1'; }
uint32_t parse_levels_8_12_16(const char* v, uint32_t) {
  const int n = atoi(v);
  return n >= 16 ? 16u : (n >= 12 ? 12u : 8u);
}
float parse_real(const char* v, float) { return (float)atof(v); }
UcsaEnvText parse_text(const char* v, UcsaEnvText) {
  UcsaEnvText t{true, {0}};
  strcpy(t.value, v);
  return t;
}

// a published snapshot; the chain keeps the earlier ones reachable
struct Snapshot {
  UcsaEnv env;
  const Snapshot* earlier;
};

const Snapshot* load(const Snapshot* earlier) {
  Snapshot* s = new Snapshot;
  s->earlier = earlier;
  UcsaEnv* e = &s->env;
#define UCSA_ENV_LOAD(name, type, field, rule, dflt)                   \
  {                                                                    \
    const char* v = getenv(name);                                      \
    e->field = v && *v && strlen(v) < 64 ? parse_##rule(v, dflt) : dflt; \
  }
  UCSA_ENV_TABLE(UCSA_ENV_LOAD)
#undef UCSA_ENV_LOAD
  return s;
}

std::atomic<const Snapshot*> current{nullptr};
std::mutex reload_mu;   // one writer at a time

const Snapshot* publish_new() {
  std::lock_guard<std::mutex> lk(reload_mu);
  const Snapshot* s = load(current.load(std::memory_order_relaxed));
  current.store(s, std::memory_order_release);
  return s;
}
}  // namespace

const UcsaEnv& ucsa_env() {
  const Snapshot* s = current.load(std::memory_order_acquire);
  if (!s) s = publish_new();   // first call (racing first calls each publish one)
  return s->env;
}

// Builds a new snapshot and publishes it with one pointer store.  The earlier
// ones stay allocated (a reader may still hold a reference): growth is one small
// struct per call, and reload is for lab tools and tests only.
extern "C" void ucsa_env_reload(void) { (void)publish_new(); }
