// match_exec_check.cpp — stand-alone host program (plain C++17, no HIP): the implication behind the tiled likelihood kernel's
// specialised pose loop (mcl_3dl_amd/csrc/likelihood_kernels.h: eval_coop_first<true>), which takes `matched` from the lanes
// that pass the radius test instead of comparing dist with 0. For every (r, flat) the launcher's predicate accepts
// (host_options.h:lik_match_from_radius) and EVERY float d2 in [0, r2), r2 = float(double(r) * r):
//     dist = r - max(RN(sqrt(d2)), flat) >= 0        (likelihood.cpp:128-132 in floats; RN = the correctly rounded root)
// and for parameters it refuses there is a d2 below r2 with dist < 0 or the parameters are not numbers — the predicate is not
// stricter than it has to be in the cases listed. One thread per radius; prints one line per radius and "all checks passed".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "host_options.h"

static float from_bits(uint32_t u)
{
  float f;
  memcpy(&f, &u, sizeof(f));
  return f;
}
static uint32_t to_bits(float f)
{
  uint32_t u;
  memcpy(&u, &f, sizeof(u));
  return u;
}

struct Case
{
  float r;
  std::vector<float> flats;   // accepted ones: flat <= r
  unsigned long long walked = 0, negative = 0;
  bool accepted = false;
};

static void walk(Case* c)
{
  const float r = c->r;
  const float r2 = static_cast<float>(static_cast<double>(r) * static_cast<double>(r));
  c->accepted = true;
  for (float flat : c->flats)
    c->accepted = c->accepted && lik_match_from_radius(r, r2, flat);
  if (!c->accepted)
    return;
  const uint32_t end = to_bits(r2);   // non-negative floats order like their bit patterns
  unsigned long long negative = 0;
  for (uint32_t u = 0; u < end; ++u)
  {
    const float s = sqrtf(from_bits(u));
    for (float flat : c->flats)
    {
      const float m = s > flat ? s : flat;   // std::max(root, flat)
      const float dist = r - m;
      negative += dist >= 0.0f ? 0u : 1u;
    }
  }
  c->walked = end;
  c->negative = negative;
}

int main()
{
  int failures = 0;
  // the reference's default (match_dist_min 0.2, match_dist_flat 0.05), a small radius of the fuzz, and awkward ones: just below a
  // power of two, one whose square is far from a float, a tiny one. flat: small, the float below r, r itself
  const float radii[] = { 0.2f, 0.05f, std::nextafterf(1.0f, 0.0f), 3.0000002f, 1.0e-3f };
  std::vector<Case> cases;
  for (float r : radii)
    cases.push_back(Case{ r, { 0.05f < r ? 0.05f : 0.25f * r, std::nextafterf(r, 0.0f), r } });
  std::vector<std::thread> pool;
  for (Case& c : cases)
    pool.emplace_back(walk, &c);
  for (std::thread& t : pool)
    t.join();
  for (const Case& c : cases)
  {
    printf("r = %.9g: accepted %d, %llu values of d2 walked x %zu flats, %llu with dist < 0\n", c.r, c.accepted ? 1 : 0, c.walked,
           c.flats.size(), c.negative);
    if (!c.accepted || c.negative != 0 || c.walked == 0)
      ++failures;
  }
  // what the predicate refuses: flat above r (dist = r - flat < 0 already at d2 = 0), and parameters that are not numbers
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float r = 0.2f, r2 = static_cast<float>(static_cast<double>(r) * static_cast<double>(r));
  struct
  {
    float r, r2, flat;
  } refused[] = { { r, r2, std::nextafterf(r, 1.0f) }, { r, r2, 0.3f }, { r, r2, nan }, { nan, nan, 0.05f } };
  for (const auto& p : refused)
  {
    const bool ok = !lik_match_from_radius(p.r, p.r2, p.flat);
    const float dist0 = p.r - (0.0f > p.flat ? 0.0f : p.flat);
    printf("refused r = %g r2 = %g flat = %g: %d (dist at d2 = 0: %g)\n", p.r, p.r2, p.flat, ok ? 1 : 0, dist0);
    if (!ok || dist0 >= 0.0f)
      ++failures;
  }
  if (failures)
  {
    printf("%d checks FAILED\n", failures);
    return 1;
  }
  printf("all checks passed\n");
  return 0;
}
