// run_loop_lifetime.cpp (TEST-ONLY) -- the lifetime of what a context allocates for its run loop, as a stand-alone program: compiled
// with rgpu_api.cpp and the host sources against tests/emu (the host emulation) under -fsanitize=address,undefined by
// tests/test_run_loop_lifetime.py.  Every leak, double free or use after free of the clock records, the history log or the monitor log
// is the sanitizer's report; every wrong return code is a message and exit status 1.
//   usage: run_loop_lifetime <directory of the .ini files>
#include <cstdio>
#include <string>
#include <vector>

#include "rgpu.h"

extern "C" void rgpu_emu_fail_launch_after(int n);   // tests/emu/rg_backend.h

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bool setup(const std::string& ini, const char* ov, rgpu_params* p, std::vector<double>* U) {
  char err[512] = "";
  if (rgpuh_params_from_ini(ini.c_str(), ov, p, err, 512)) { std::fprintf(stderr, "params_from_ini: %s\n", err); return false; }
  const size_t gw = (size_t)p->ghostWidth, nk = p->nz_global != 1 ? p->nz + 2 * gw : 1;
  U->assign((size_t)p->nbVar * nk * (p->ny + 2 * gw) * (p->nx + 2 * gw), 0.0);
  if (rgpuh_init_condition(ini.c_str(), ov, p, U->data(), err, 512)) { std::fprintf(stderr, "init_condition: %s\n", err); return false; }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string configs = argv[1];
  rgpu_params p;
  std::vector<double> U;

  // a lone 3D MHD context through all three loops: every mirror is allocated, the plain run crosses a batch boundary
  if (!setup(configs + "/mhd_mri_3d.ini", "mesh.nx=8;mesh.ny=8;mesh.nz=8", &p, &U)) return 1;
  rgpu_ctx* c = 0;
  EXPECT(rgpu_create(&p, &c) == RGPU_OK);
  EXPECT(rgpu_upload(c, U.data(), 1) == RGPU_OK);
  int nStep = 0, hn = 0, mn = 0;
  double t = 0.0, dt = 0.0, tHist = 0.0;
  std::vector<int> step(300);
  std::vector<double> ts(300), dts(300), rows(300 * RGPU_HIST_NQ), mon(300 * RGPU_MON_NQ), log(300);
  EXPECT(rgpu_run_steps_history(c, 10, 1e300, &nStep, &t, &dt, log.data(), 0.0, &tHist, &hn, step.data(), ts.data(), dts.data(), rows.data()) == 10);
  EXPECT(hn == 10 && rgpu_history_batch_heads(c) == 9);
  EXPECT(rgpu_run_steps_monitored(c, 10, 1e300, &nStep, &t, &dt, log.data(), 2, &mn, step.data(), ts.data(), mon.data()) == 10);
  EXPECT(mn == 5 && rgpu_monitor_batch_samples(c) == 5);
  EXPECT(rgpu_run_steps(c, 300, 1e300, &nStep, &t, &dt) == 300);
  EXPECT(nStep == 320);
  // a launch that fails inside a batch: the steps queued in front of it ran and are counted, the call reports the failure
  rgpu_emu_fail_launch_after(6);
  EXPECT(rgpu_run_steps_monitored(c, 8, 1e300, &nStep, &t, &dt, log.data(), 2, &mn, step.data(), ts.data(), mon.data()) == RGPU_EHIP);
  rgpu_emu_fail_launch_after(0);
  EXPECT(nStep == 321 && mn == 0);
  rgpu_destroy(c);

  // a two-member 2D ensemble: members are contexts over slices of its storage and go with it
  if (!setup(configs + "/orszag-tang.ini", "mesh.nx=8;mesh.ny=8", &p, &U)) return 1;
  rgpu_ensemble* e = 0;
  EXPECT(rgpu_ensemble_create(&p, 2, &e) == RGPU_OK);
  for (int m = 0; m < 2; ++m) EXPECT(rgpu_upload(rgpu_ensemble_member(e, m), U.data(), 1) == RGPU_OK);
  int n2[2] = {0, 0}, done[2] = {0, 0};
  double t2[2] = {0.0, 0.0}, dt2[2] = {0.0, 0.0};
  EXPECT(rgpu_ensemble_run_steps(e, 5, 0, n2, t2, dt2, 0, done, 0, 0) == RGPU_OK);
  EXPECT(done[0] == 5 && done[1] == 5 && t2[0] == t2[1]);
  rgpu_destroy(rgpu_ensemble_member(e, 0));   // refused: the member belongs to the ensemble
  rgpu_ensemble_destroy(e);

  // a context whose creation was refused is still returned, and destroyed like any other
  p.abi_version += 1;
  c = 0;
  EXPECT(rgpu_create(&p, &c) == RGPU_EINVAL && c != 0);
  rgpu_destroy(c);

  if (failures) return 1;
  std::puts("run_loop_lifetime: ok");
  return 0;
}
