// options_check.cpp — the option table of mcl_3dl_amd/csrc/host_options.h checked on the CPU, with that header alone (no HIP, no
// library): tests/test_options_table.py builds it (-std=c++17 -Wall -Werror) and passes the value pool of the API fuzz,
// one argument per key: name=v1,v2,... Prints one line per row — "<name> <default> <read-back of each pool value>..." — and
// exits non-zero when a check fails.
#include <cmath>
#include <string>
#include <vector>

#include "host_options.h"

namespace
{
int g_bad = 0;
#define CHECK(cond, ...)                   \
  do                                       \
  {                                        \
    if (!(cond))                           \
    {                                      \
      ++g_bad;                             \
      printf("FAILED %s: ", #cond);        \
      printf(__VA_ARGS__);                 \
      printf("\n");                        \
    }                                      \
  } while (0)

constexpr size_t N = sizeof(kOptions) / sizeof(kOptions[0]);

// the stored value of a row's field, the hook's included (option_get refuses that one)
double stored(const Options& o, const OptionRow& r)
{
  return option_load(o, r.field);
}

std::vector<double> snapshot(const Options& o)
{
  std::vector<double> s;
  for (const OptionRow& r : kOptions)
    s.push_back(stored(o, r));
  return s;
}

void rejected(const char* name, double v)
{
  Options o;
  const std::vector<double> before = snapshot(o);
  const OptionSet s = option_set(o, name, v);
  const std::string want = std::string(name) + " must ";
  CHECK(s.code == -3 && s.effects == 0u, "%s = %g: code %d, effects %u", name, v, s.code, s.effects);
  CHECK(std::string(s.msg).compare(0, want.size(), want) == 0 && strlen(s.msg) > want.size(), "%s = %g: '%s'", name, v, s.msg);
  CHECK(snapshot(o) == before, "%s = %g was refused and changed a field", name, v);
}
}  // namespace

int main(int argc, char** argv)
{
  setenv("MCL3DL_HIP_TEST_HOOKS", "1", 1);
  const Options defaults;
  for (size_t a = 0; a < N; ++a)
  {
    const OptionRow& r = kOptions[a];
    for (size_t b = 0; b < a; ++b)
      CHECK(strcmp(r.name, kOptions[b].name) != 0, "rows %zu and %zu are both '%s'", b, a, r.name);
    // its own default: accepted, nothing changes, no effect beyond the row's unconditional one
    Options o;
    const OptionSet s = option_set(o, r.name, stored(defaults, r));
    CHECK(s.code == 0 && s.effects == r.always, "%s at its default: code %d '%s', effects %u", r.name, s.code, s.msg, s.effects);
    CHECK(snapshot(o) == snapshot(defaults), "%s at its default changed a field", r.name);
    double back = -7;
    CHECK(option_get(o, r.name, &back) == !r.test_hook, "%s: readable %d", r.name, !r.test_hook);
    CHECK(r.test_hook || back == stored(defaults, r), "%s reads %g", r.name, back);
    // NaN: a flag stores 1, every other rule refuses it
    if (r.rule.flag)
    {
      CHECK(option_set(o, r.name, NAN).code == 0 && stored(o, r) == 1.0, "%s = NaN stores %g", r.name, stored(o, r));
    }
    else
      rejected(r.name, NAN);

    printf("%s %.17g", r.name, stored(defaults, r));
    // the fuzz's pool: every value accepted, the read-back is the stored conversion
    for (int k = 1; k < argc; ++k)
    {
      const std::string arg(argv[k]);
      const size_t eq = arg.find('=');
      if (eq == std::string::npos || arg.substr(0, eq) != r.name)
        continue;
      const char* p = arg.c_str() + eq + 1;
      while (*p)
      {
        char* end = nullptr;
        const double v = strtod(p, &end);
        CHECK(end != p, "%s: cannot parse '%s'", r.name, p);
        if (end == p)
          break;
        p = *end == ',' ? end + 1 : end;
        const OptionSet sv = option_set(o, r.name, v);
        CHECK(sv.code == 0, "%s = %g: '%s'", r.name, v, sv.msg);
        const double want = r.rule.flag ? static_cast<double>(v != 0.0) : r.field.type == OptionField::Int ? std::trunc(v) : v;
        back = -7;
        CHECK(option_get(o, r.name, &back) && back == want && stored(o, r) == want, "%s = %g reads %g", r.name, v, back);
        printf(" %.17g", back);
      }
    }
    printf("\n");
  }

  // values outside the rules: refused, nothing touched
  rejected("lik_index", 7);
  rejected("lik_group", 5);
  rejected("cand_phase", 1.0);
  rejected("cand_voxel_ratio", 0.1);
  rejected("strict_chunk", 512);
  rejected("index_budget_bytes", -2);
  rejected("batch_slice", NAN);
  rejected("batch_slice", -1);
  rejected("timing_mask", -1);
  rejected("timing_mask", 4294967296.0);

  // conversions and effects
  {
    Options o;
    CHECK(option_set(o, "lik_tiled_min", 1.5).code == 0 && o.lik_tiled_min == 1, "lik_tiled_min 1.5 stores %d", o.lik_tiled_min);
    CHECK(option_set(o, "timing_mask", 4294967295.0).code == 0 && o.timing_mask == 0xffffffffu, "timing_mask %u", o.timing_mask);
    CHECK(option_set(o, "update_small", -0.5).code == 0 && o.update_small == 1, "a flag stores value != 0");
    CHECK(option_set(o, "lik_defer", 2).effects == EFFECT_CAND && option_set(o, "lik_defer", 2).effects == 0u, "lik_defer: on change only");
    CHECK(option_set(o, "cand_phase", 0.25).effects == EFFECT_CAND && option_set(o, "cand_phase", 0.25).effects == 0u, "cand_phase");
    CHECK(option_set(o, "grid_build_host", 3).effects == EFFECT_GRIDS && option_set(o, "grid_build_host", 1).effects == 0u, "grid_build_host");
    CHECK(option_set(o, "dda_overlay", 1).effects == EFFECT_DDA && option_set(o, "dda_overlay", 0).effects == EFFECT_DDA, "dda_overlay: always");
    CHECK(option_set(o, "strict_order", 3).effects == 0u && o.strict_order == 3, "strict_order");
    const OptionSet s = option_set(o, "no_such_option", 1);
    CHECK(s.code == -3 && strcmp(s.msg, "unknown option 'no_such_option'") == 0, "'%s'", s.msg);
    double v;
    CHECK(!option_get(o, "no_such_option", &v) && !option_get(o, "lik_exact", &v), "only the table's keys are read here");
  }

  // the hook: refused unless the environment enables it
  {
    Options o;
    unsetenv("MCL3DL_HIP_TEST_HOOKS");
    OptionSet s = option_set(o, "test_late_structures", 1);
    CHECK(s.code == -3 && !o.test_late_structures && strstr(s.msg, "is a test hook"), "hook without the variable: %d '%s'", s.code, s.msg);
    setenv("MCL3DL_HIP_TEST_HOOKS", "0", 1);
    CHECK(option_set(o, "test_late_structures", 1).code == -3 && !test_hooks_enabled(), "hook with the variable at 0");
    setenv("MCL3DL_HIP_TEST_HOOKS", "1", 1);
    s = option_set(o, "test_late_structures", 1);
    CHECK(s.code == 0 && o.test_late_structures && s.effects == 0u, "hook with the variable: %d '%s'", s.code, s.msg);
  }

  printf("options_check: %zu rows, %s\n", N, g_bad ? "FAILED" : "all checks passed");
  return g_bad ? 1 : 0;
}
