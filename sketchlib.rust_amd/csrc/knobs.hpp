// knobs.hpp -- the environment switches as a plain struct, and the reader that fills it from a lookup function.  Both expand from
// the one table knobs.def.  No HIP header: the launch plans (dense_plan.hpp, knn_plan.hpp) and the CPU tests read it without a device
// toolchain.  capi_internal.hpp includes it; capi_knobs.cpp read_knobs() hands knobs_from() the process environment.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

// Environment switches.  They are read when a context is created (skl_ctx_create) or asked to look again (skl_ctx_reload_env),
// never on the launch path.  The struct has ONE layout in both builds; the product library reads the entries of class PRODUCT and
// leaves every A/B entry -- kernel selection, tile shapes, the timing-only ablations, every "results identical" comparison -- at
// its default, which is what the plans then see.
struct Knobs {
#define KNOB_INT(cls, type, field, name, dflt, lo, hi, desc) type field = dflt;
#define KNOB_INT_UNLESS_0(cls, type, field, name, lo, desc) type field = 0;
#define KNOB_WORD(cls, field, name, word, desc) bool field = false;
#define KNOB_CHOICE(cls, field, name, word_a, value_a, word_b, value_b, desc) int field = 0;
#include "knobs.def"
};

using KnobLookup = const char *(*)(const char *name);   // the variable's text, or null: the C library's lookup, or a test's map

constexpr long long KNOB_NO_LOW = LLONG_MIN, KNOB_NO_HIGH = LLONG_MAX;

// an empty string counts as unset; text that is no number goes through atoll (0, or its leading digits)
inline long long knob_int(KnobLookup look, const char *name, long long dflt, long long lo = KNOB_NO_LOW, long long hi = KNOB_NO_HIGH)
{
    const char *e = look(name);
    return std::min(hi, std::max(lo, (e && *e) ? atoll(e) : dflt));
}
inline bool knob_is(KnobLookup look, const char *name, const char *word)
{
    const char *e = look(name);
    return e && strcmp(e, word) == 0;
}

// An A/B entry's read -- and with it the variable's name -- exists in the A/B build alone.
#define KNOB_READ_PRODUCT(statement) statement
#ifdef SKL_AB
#define KNOB_READ_AB(statement) statement
#else
#define KNOB_READ_AB(statement)
#endif

inline Knobs knobs_from(KnobLookup look)
{
    Knobs k;
#define KNOB_INT(cls, type, field, name, dflt, lo, hi, desc) KNOB_READ_##cls(k.field = static_cast<type>(knob_int(look, name, dflt, lo, hi));)
#define KNOB_INT_UNLESS_0(cls, type, field, name, lo, desc) \
    KNOB_READ_##cls(k.field = static_cast<type>(knob_int(look, name, 0)); if (k.field != 0) k.field = std::max<type>(lo, k.field);)
#define KNOB_WORD(cls, field, name, word, desc) KNOB_READ_##cls(k.field = knob_is(look, name, word);)
#define KNOB_CHOICE(cls, field, name, word_a, value_a, word_b, value_b, desc) \
    KNOB_READ_##cls(k.field = knob_is(look, name, word_a) ? value_a : knob_is(look, name, word_b) ? value_b : 0;)
#include "knobs.def"
    return k;
}

#undef KNOB_READ_PRODUCT
#undef KNOB_READ_AB
