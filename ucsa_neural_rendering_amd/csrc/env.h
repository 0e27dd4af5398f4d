// The library's environment switches ("Environment variables"):
// ONE table, parsed into one typed snapshot.  Every switch is a launch shape /
// kernel choice, never a result.  Plain C++ (no HIP): env.cpp builds alone.
#pragma once
#include <stdint.h>

#include "ucsa_hip.h"

// UCSA_ENC_ORDER stays text: its meaning depends on the grid's level count
// (hashgrid.hip, level_map), and its mere presence matters.
struct UcsaEnvText {
  bool present;
  char value[64];
};

// One row per switch: X(name, field type, field, parse rule, default).  The
// rules are env.cpp's parse_* functions; a value that is empty or 64 or more
// characters long counts as unset, and unset gives the default.
#define UCSA_ENV_TABLE(X)                                                       \
  /* launch shapes / kernel choices of the render path */                       \
  X("UCSA_ENC_SORTED", int32_t, enc_sorted, digit_0_to_4, 2)                    \
  X("UCSA_ENC_ML", int32_t, enc_ml, integer, -1) /* negative: no override */    \
  X("UCSA_ENC_SORTED_ML", uint32_t, enc_sorted_ml, unsigned_integer, 9u)        \
  X("UCSA_DENSITY_FUSED", bool, density_fused, on_unless_0, true)               \
  X("UCSA_DENSITY_LEVELS", uint32_t, density_levels, levels_8_12_16, 12u)       \
  /* ... of the training path */                                                \
  X("UCSA_SHADE_BWD_SPLIT", bool, shade_bwd_split, on_unless_0, true)           \
  X("UCSA_BWD_OVERLAP", bool, bwd_overlap, on_unless_0, true)                   \
  X("UCSA_BWD_BIN_SCALE", float, bwd_bin_scale, real, 100.0f)                   \
  /* lab only (tools/encode_*.py) */                                            \
  X("UCSA_ENC_ORDER", UcsaEnvText, enc_order, text, UcsaEnvText{})              \
  X("UCSA_ENC_SIMPLE", uint32_t, enc_simple, unsigned_integer, UCSA_MAX_LEVELS) \
  X("UCSA_ENC_SIMPLE_H", uint32_t, enc_simple_h, unsigned_integer, 0u)          \
  X("UCSA_ENC_SIMPLE_RAYS", uint32_t, enc_simple_rays, unsigned_integer, 0u)    \
  X("UCSA_SORT_EXACT", bool, sort_exact, on_unless_0, true)                     \
  /* lab only (tools/components_time.py): the lattice labelling without its LDS stage */ \
  X("UCSA_COMPONENTS_NO_LDS", bool, components_no_lds, on_if_1, false)

struct UcsaEnv {
#define UCSA_ENV_FIELD(name, type, field, rule, dflt) type field;
  UCSA_ENV_TABLE(UCSA_ENV_FIELD)
#undef UCSA_ENV_FIELD
};

// The current snapshot: read from the environment at the first call, replaced
// as a whole by ucsa_env_reload() (lab tools and tests that flip a switch inside
// one process).  A snapshot is never written after it is published and never
// freed, so a reference stays valid and consistent, whatever thread holds it;
// consumers read a field per call and keep no copy in a static.
const UcsaEnv& ucsa_env();
