// Walks the argument checks of the thermal entry points (slf_thermal_*; sailfish_amd/csrc/slf_bind.h thermal_check) on the CPU
// and prints one line per case:  subject <tab> code <tab> message.
// tests/test_thermal_bind.py builds it stand-alone (no GPU, nothing loaded into Python) and reads the lines.
#include <math.h>
#include <stdio.h>

#include <string>

#include "bind_desc.h"
#include "slf_bind.h"

namespace {

slf_module_desc base_desc(int lattice) {
  slf_module_desc d = bind_fluid_only_desc(lattice);
  d.accel_field = (lattice == SLF_D2Q9 || lattice == SLF_D3Q19) ? 1 : 0;
  return d;
}

struct Call {
  bool has_field = true;
  slf_thermal_params params = {1.25, 0.5, {0.0, 1e-3, 0.0}, {1, 0, 0}, 0};
  const slf_thermal_params* params_ptr = &params;
  int a = 0, b = 0;
  const void* map = nullptr;
  const void* ptrs[2] = {&a, &b};
  const void* src = &a;
  const void* dst = &b;
};

int line(const char* subject, const slf_module_desc& d, const Call& call) {
  slf::ModuleConfig c;
  const char* why = "";
  if (slf::module_config(&d, &c, &why)) {
    printf("%s\t-1\tmodule_config: %s\n", subject, why);
    return 1;
  }
  static const char* const names[2] = {"g_src", "T"};
  std::string err;
  const int rc = slf::thermal_check(c, call.has_field, "slf_thermal_test", call.params_ptr, call.map, call.ptrs, names, 2, call.src,
                                    call.dst, &err);
  printf("%s\t%d\t%s\n", subject, rc, err.c_str());
  return 0;
}

slf_module_desc with_node_types(slf_module_desc d) {
  d.fluid_only = 0;
  d.n_types = 3;
  d.type_kind[0] = SLF_NK_FLUID; d.type_kind[1] = SLF_NK_GHOST; d.type_kind[2] = SLF_NK_FULL_BB;
  d.nt_type_mask = 15; d.nt_misc_shift = 4; d.nt_param_shift = 3; d.nt_scratch_shift = 0;
  return d;
}

}  // namespace

int main() {
  int bad = 0;
  bad += line("served-d2q9", base_desc(SLF_D2Q9), Call());
  {
    slf_module_desc d = base_desc(SLF_D3Q19);
    d.precision = 8; d.model = SLF_MRT; d.access_pattern = SLF_AA;
    Call c; c.params.omega_T = 1.999; c.params.T_ref = -3.0; c.src = nullptr; c.dst = nullptr;       // (init: one copy)
    bad += line("served-d3q19-f64", d, c);
  }
  { Call c; c.map = &c.a; bad += line("served-with-map", with_node_types(base_desc(SLF_D3Q19)), c); }
  { slf_module_desc d = base_desc(SLF_D3Q19); d.accel_field = 0; bad += line("no-accel-field", d, Call()); }
  { Call c; c.has_field = false; bad += line("field-not-set", base_desc(SLF_D3Q19), c); }
  { Call c; c.params_ptr = nullptr; bad += line("null-params", base_desc(SLF_D3Q19), c); }
  { Call c; c.params.omega_T = 0.0; bad += line("omega-zero", base_desc(SLF_D2Q9), c); }
  { Call c; c.params.omega_T = 2.0; bad += line("omega-two", base_desc(SLF_D2Q9), c); }
  { Call c; c.params.omega_T = -0.5; bad += line("omega-negative", base_desc(SLF_D2Q9), c); }
  { Call c; c.params.omega_T = NAN; bad += line("omega-nan", base_desc(SLF_D2Q9), c); }
  { Call c; c.params.b[1] = INFINITY; bad += line("buoyancy-not-finite", base_desc(SLF_D2Q9), c); }
  { Call c; c.params.T_ref = NAN; bad += line("t-ref-nan", base_desc(SLF_D2Q9), c); }
  bad += line("null-map-with-node-types", with_node_types(base_desc(SLF_D3Q19)), Call());
  { Call c; c.ptrs[0] = nullptr; bad += line("null-g-src", base_desc(SLF_D2Q9), c); }
  { Call c; c.ptrs[1] = nullptr; bad += line("null-t", base_desc(SLF_D2Q9), c); }
  { Call c; c.dst = c.src; bad += line("src-is-dst", base_desc(SLF_D3Q19), c); }
  bad += line("d3q15", base_desc(SLF_D3Q15), Call());
  bad += line("d3q27", base_desc(SLF_D3Q27), Call());
  return bad ? 2 : 0;
}
