// sac_form_host.cpp — the SAC step-form decision (ilswiss_amd/csrc/sac_form.h) and the switch table (switches.h) on the host: the form functions
// against callables that count their calls, next to the three predicates they replaced, restated literally; the switch accessors against a stub
// environment.  tests/test_sac_form_host.py drives it through the C entry points at the end.
#include <map>
#include <string>

static std::map<std::string, std::string> g_env;
static const char* stub_env(const char* name) {
  auto it = g_env.find(name);
  return it == g_env.end() ? nullptr : it->second.c_str();
}
#define ILSX_SWITCH_ENV(name) stub_env(name)
#include "../../ilswiss_amd/csrc/sac_form.h"
#include "../../ilswiss_amd/csrc/switches.h"

// one combination of inputs, as bits
enum { IN_WIDE = 1, IN_COL = 2, IN_BROKEN = 4, IN_SPLIT = 8, IN_NO_PHASE = 16, IN_NO_FUSE = 32, IN_FITS = 64, IN_HEADS = 128, IN_OWN = 256, IN_DEFER = 512 };

// The predicates as they stood before sac_form.h, term for term in their order (ilsx_sac.hip: sac_phase_ok, sac_phase_possible,
// sac_window_may_use_phase), on plain values.
static bool old_phase_ok(bool off, bool phase_broken, int cs, bool h0scr, bool col, bool defer_tail, int xcd_shift, bool phase_fits, bool static_heads) {
  return !off && !phase_broken && cs > 1 && !h0scr && !col && defer_tail && xcd_shift == 0 && phase_fits && static_heads;
}
static bool old_phase_possible(bool off, int cs, bool h0scr, bool phase_fits, bool static_heads) {
  return !off && cs > 1 && !h0scr && phase_fits && static_heads;
}
static bool old_window_may_use_phase(bool off, bool phase_broken, int cs, bool h0scr, bool col, int xcd_shift, bool phase_fits, bool static_heads) {
  return !phase_broken && cs > 1 && !col && old_phase_possible(off, cs, h0scr, phase_fits, static_heads) && xcd_shift == 0;
}

extern "C" {
// out[0..2]: the window answer and the calls of phase_fits / static_heads it made; out[3..5]: the same for the step answer; out[6]: the calls of
// phase_own_rows that sac_step_form made; out[7..10]: that form's fuse, defer_tail, phase, own_rows; out[11..13]: the old sac_phase_ok,
// sac_phase_possible, sac_window_may_use_phase
void sfh_decide(int cs, int xcd_shift, int bits, int* out) {
  int n_fits = 0, n_heads = 0, n_own = 0;
  SacFormInputs in;
  in.cs = cs; in.xcd_shift = xcd_shift;
  in.wide_l0 = bits & IN_WIDE; in.collecting = bits & IN_COL; in.phase_broken = bits & IN_BROKEN; in.split = bits & IN_SPLIT;
  in.no_phase = bits & IN_NO_PHASE; in.no_fuse = bits & IN_NO_FUSE;
  in.phase_fits = [&] { ++n_fits; return (bits & IN_FITS) != 0; };
  in.static_heads = [&] { ++n_heads; return (bits & IN_HEADS) != 0; };
  in.phase_own_rows = [&] { ++n_own; return (bits & IN_OWN) != 0; };
  const bool defer = bits & IN_DEFER;
  out[0] = sac_window_may_phase(in); out[1] = n_fits; out[2] = n_heads;
  n_fits = n_heads = n_own = 0;
  out[3] = sac_step_may_phase(in, defer); out[4] = n_fits; out[5] = n_heads;
  n_fits = n_heads = n_own = 0;
  const SacStepForm f = sac_step_form(in, defer, nullptr);
  out[6] = n_own;
  out[7] = f.fuse; out[8] = f.defer_tail; out[9] = f.phase; out[10] = f.own_rows;
  const bool off = in.no_phase, fits = bits & IN_FITS, heads = bits & IN_HEADS;
  out[11] = old_phase_ok(off, in.phase_broken, cs, in.wide_l0, in.collecting, defer, xcd_shift, fits, heads);
  out[12] = old_phase_possible(off, cs, in.wide_l0, fits, heads);
  out[13] = old_window_may_use_phase(off, in.phase_broken, cs, in.wide_l0, in.collecting, xcd_shift, fits, heads);
}
// two default forms that differ in field `k` only: 1 when == and != see exactly that (and a form equals itself)
int sfh_form_compares(int k) {
  static int ring_stand_in, col_stand_in;
  SacStepForm a, b;
  switch (k) {
    case 0: b.ring = (ilsx_replay*)&ring_stand_in; break;
    case 1: b.col = (SacCollector*)&col_stand_in; break;
    case 2: b.fuse = true; break;
    case 3: b.defer_tail = true; break;
    case 4: b.phase = true; break;
    case 5: b.own_rows = true; break;
    case 6: b.mode = SAC_FORM_UPLOAD; break;
    case 7: b.mode = SAC_FORM_CHECK; break;
    default: return a == b && !(a != b);   // no difference
  }
  return a == a && b == b && a != b && !(a == b);
}

void sfh_setenv(const char* name, const char* value) { if (value) g_env[name] = value; else g_env.erase(name); }
// parse rules by name: 0 PRESENT, 1 UNLESS0, 2 INT
int sfh_parse(int rule, const char* value, int dflt) {
  return rule == 0 ? (int)sw::parse_PRESENT(value, dflt) : rule == 1 ? (int)sw::parse_UNLESS0(value, dflt) : sw::parse_INT(value, dflt);
}
// the accessor of the row `name`, as an int; -12345 for a name the table does not have
int sfh_switch(const char* name) {
#define SFH_ROW(n, rule, dflt, life, meaning) if (std::string(name) == #n) return (int)sw::n();
  ILSX_SWITCHES(SFH_ROW)
#undef SFH_ROW
  return -12345;
}
}
