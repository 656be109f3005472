// Host compilation of the arithmetic of the group velocities on the device (pinocchio_amd/csrc/pf_groupvel_core.h, with the cell
// arithmetic of pf_refresh_core.h) for tests/test_groupvel_cpu.py: the three classes of a particle, the key of a counted one, the
// sorted keys with their head flags and slots, and the sums walked as the kernels of pf_groupvel.hip walk them -- unit by unit, the
// units of a tile combined in order (pf_gv_combine), the carries folded in tile order (pf_gv_fold) -- for any unit and tile size, so
// that segments start, end and span units and tiles.  (Inside a unit the device adds in a tree of shuffles, this file from left to
// right: the sums agree exactly where they are exact, and within the bound of fp64 summation otherwise.)
// port_group_velocities is recompute_group_velocities() (src/fragment.c:852-909) restated in plain C: a float running sum along the
// linking list of every group, all eight fields zeroed first, divided by (double) Mass.  The file is a program: its main holds the
// two against each other; it is also built under -fsanitize=address,undefined.  -DGROUPVEL_EMUL_LIB leaves the main out (the shared
// object the test loads).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../pinocchio_amd/csrc/pf_distribute_boxes.h"
#include "../../pinocchio_amd/csrc/pf_refresh_core.h"
#include "../../pinocchio_amd/csrc/pf_groupvel_core.h"
#include "large_boxes.h"

static PfBackBox box_of(int n, int x0, int nxl, const int *start, const int *len, const int *safe) {
  PfBackBox b;
  for (int d = 0; d < 3; d++) { b.box.len[d] = len[d]; b.box.pbc[d] = len[d] == n; b.box.safe[d] = safe[d]; b.start[d] = pf_dist_wrap(start[d], n); }
  b.n = n; b.x0 = x0; b.nxl = nxl;
  return b;
}

extern "C" {

// per particle: 0 not found, 1 loose, 2 counted
void emul_classes(int n, int x0, int nxl, const int *start, const int *len, const int *safe, size_t count, const unsigned int *pos, const int *gid, int first_group,
                  unsigned char *cls) {
  const PfBackBox b = box_of(n, x0, nxl, start, len, safe);
  for (size_t i = 0; i < count; i++) {
    size_t a;
    cls[i] = !pf_refresh_cell(b, pos[i], &a) ? 0 : gid[i] < first_group ? 1 : 2;
  }
}

// key packing there and back: 0 when every (gid, cell) comes back from its key and the keys order as (gid, cell)
int emul_keys(size_t count, const unsigned int *gid, const unsigned long long *cell, unsigned long long ncell) {
  const unsigned int cb = pf_gv_bits(ncell - 1);
  for (size_t i = 0; i < count; i++) {
    const unsigned long long k = pf_gv_key(gid[i], cell[i], cb);
    if (pf_gv_group(k, cb) != gid[i] || pf_gv_cell(k, cb) != cell[i]) return 1;
    if (i) {
      const unsigned long long k0 = pf_gv_key(gid[i - 1], cell[i - 1], cb);
      const bool lt = gid[i - 1] < gid[i] || (gid[i - 1] == gid[i] && cell[i - 1] < cell[i]);
      if (lt != (k0 < k)) return 2;
    }
  }
  return 0;
}

// the sums as the kernels build them: cols24 = 24 columns of ncell doubles; units of `unit` keys, `units` of them a tile.  group /
// npart / sum24 have room for count entries.  Returns the number of groups; *counted = the counted particles
unsigned long long emul_group_sums(int n, int x0, int nxl, const int *start, const int *len, const int *safe, size_t count, const unsigned int *pos, const int *gid,
                                   int first_group, const double *cols24, int unit, int units, int *group, unsigned int *npart, double *sum24,
                                   unsigned long long *counted) {
  const PfBackBox b = box_of(n, x0, nxl, start, len, safe);
  const size_t ncell = (size_t)nxl * n * n;
  const unsigned int cb = pf_gv_bits(ncell - 1);
  std::vector<unsigned long long> keys;
  for (size_t i = 0; i < count; i++) {   // k_groupvel_flag, k_groupvel_keys
    size_t a;
    if (pf_refresh_cell(b, pos[i], &a) && gid[i] >= first_group) keys.push_back(pf_gv_key((unsigned int)gid[i], a, cb));
  }
  std::sort(keys.begin(), keys.end());
  const unsigned long long m = keys.size();
  *counted = m;
  if (!m) return 0;
  std::vector<unsigned int> slot(m);     // k_groupvel_heads and the scan
  unsigned int heads = 0;
  for (unsigned long long j = 0; j < m; j++) { heads += pf_gv_head(keys.data(), j, cb); slot[j] = heads - 1; }
  const unsigned long long tile = (unsigned long long)unit * units, ntiles = (m + tile - 1) / tile;
  std::vector<double> carryF(ntiles * PF_GV_NV, NAN), carryL(ntiles * PF_GV_NV, NAN), F((size_t)units * PF_GV_NV), L((size_t)units * PF_GV_NV);
  std::vector<unsigned int> slotL(ntiles, 0xFFFFFFFFu), tflags(ntiles, 0xFFFFFFFFu), uslot(units), uflags(units);
  for (unsigned int s = 0; s < heads; s++) { npart[s] = 0xFFFFFFFFu; for (int k = 0; k < 24; k++) sum24[24 * (size_t)s + k] = NAN; }
  PfGvOut o;
  o.sum = sum24; o.npart = npart; o.carryF = carryF.data(); o.carryL = carryL.data(); o.slotL = slotL.data(); o.tflags = tflags.data();
  for (unsigned long long t = 0; t < ntiles; t++) {   // k_groupvel_reduce
    for (int u = 0; u < units; u++) {
      uflags[u] = 0;
      const unsigned long long a = t * tile + (unsigned long long)u * unit, e = a + unit < m ? a + unit : m;
      if (a >= m) continue;
      double v[PF_GV_NV];
      bool began_here = false;
      if (!pf_gv_head(keys.data(), a, cb)) uflags[u] |= PF_GV_HAS_F;
      for (unsigned long long j = a; j < e; j++) {
        const bool head = pf_gv_head(keys.data(), j, cb), tail = pf_gv_tail(keys.data(), m, j, cb);
        const size_t addr = (size_t)pf_gv_cell(keys[j], cb);
        if (head || j == a) for (int k = 0; k < PF_GV_NV; k++) v[k] = 0.0;
        if (head) { began_here = true; group[slot[j]] = (int)pf_gv_group(keys[j], cb); }
        for (int k = 0; k < 24; k++) v[k] = (head || j == a) ? cols24[(size_t)k * ncell + addr] : v[k] + cols24[(size_t)k * ncell + addr];
        v[24] += 1.0;
        if (tail) {
          if (began_here) for (int k = 0; k < PF_GV_NV; k++) pf_gv_emit(o, slot[j], k, v[k]);
          else { for (int k = 0; k < PF_GV_NV; k++) F[(size_t)PF_GV_NV * u + k] = v[k]; uflags[u] |= PF_GV_F_CLOSES; }
        } else if (j + 1 == e) {
          if (began_here) { for (int k = 0; k < PF_GV_NV; k++) L[(size_t)PF_GV_NV * u + k] = v[k]; uslot[u] = slot[j]; uflags[u] |= PF_GV_HAS_L; }
          else for (int k = 0; k < PF_GV_NV; k++) F[(size_t)PF_GV_NV * u + k] = v[k];
        }
      }
    }
    for (int k = 0; k < PF_GV_NV; k++) pf_gv_combine(o, t, units, F.data(), L.data(), uslot.data(), uflags.data(), k);
  }
  for (unsigned long long t = 0; t < ntiles; t++)   // k_groupvel_fold
    for (int k = 0; k < PF_GV_NV; k++) pf_gv_fold(o, t, ntiles, k);
  return heads;
}

// recompute_group_velocities(), :852-909, for PRODFLOAT = float.  frag: Nstored records of 24 floats (Vel, Vel_2LPT, Vel_3LPT_1,
// Vel_3LPT_2, then their *_prev); groups 0 .. ngroups with point, Mass and the same 24 floats; all eight fields are zeroed (the
// reference zeroes Vel_prev twice and Vel_2LPT_prev never, :863)
struct PortGroup { int point, Mass; float v[24]; };
void port_group_velocities(int ngroups, PortGroup *groups, const float *frag, const int *linking_list, int first_group) {
  for (int i = first_group; i <= ngroups; i++)
    if (groups[i].point >= 0 && groups[i].Mass > 0) {
      for (int k = 0; k < 24; k++) groups[i].v[k] = 0;
      int next = groups[i].point;
      for (int npart = 0; npart < groups[i].Mass; npart++) {
        for (int k = 0; k < 24; k++) groups[i].v[k] += frag[24 * (size_t)next + k];
        next = linking_list[next];
      }
      for (int k = 0; k < 24; k++) groups[i].v[k] /= (double)groups[i].Mass;
    }
}
}

#ifndef GROUPVEL_EMUL_LIB
struct Case { int n, x0, nxl, start[3], len[3], safe[3]; };

int main() {
  const Case cases[] = {{16, 0, 16, {0, 0, 0}, {16, 16, 16}, {0, 0, 0}}, {16, 0, 16, {-3, 0, 13}, {7, 16, 5}, {1, 0, 1}},
                        {24, 0, 24, {20, 3, 0}, {9, 5, 24}, {2, 1, 0}},  {8, 0, 8, {6, 2, 5}, {4, 3, 5}, {1, 1, 2}}};
  const int shapes[][2] = {{1, 2}, {3, 1}, {16, 4}, {64, 16}};   // (unit, units): tiles of 2, 3, 64 and the device's 1024
  unsigned long long seed = 4242;
  auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (unsigned int)(seed >> 33); };
  for (const Case &cs : cases) {
    const size_t cells = (size_t)cs.len[0] * cs.len[1] * cs.len[2], ncell = (size_t)cs.nxl * cs.n * cs.n;
    const PfBackBox b = box_of(cs.n, cs.x0, cs.nxl, cs.start, cs.len, cs.safe);
    // every position once, in random order (the slab is the box: every particle is found); groups of random sizes, a fifth loose
    std::vector<unsigned int> pos(cells);
    for (size_t i = 0; i < cells; i++) pos[i] = (unsigned int)i;
    for (size_t i = cells; i > 1; i--) { const size_t j = rnd() % i; std::swap(pos[i - 1], pos[j]); }
    const int ngroups = 2 + (int)(cells / 40);
    std::vector<int> gid(cells);
    for (size_t i = 0; i < cells; i++) gid[i] = rnd() % 5 == 0 ? (int)(rnd() % 2) : 2 + (int)((rnd() % ngroups) * (unsigned long long)(rnd() % ngroups) / ngroups);
    for (size_t i = 0; i < cells; i++) if (gid[i] > ngroups) gid[i] = ngroups;
    std::vector<float> colsf(24 * ncell);
    std::vector<double> cols(24 * ncell);
    for (size_t q = 0; q < 24 * ncell; q++) { colsf[q] = ((float)(rnd() % 2000001) - 1000000.0f) * 1e-4f * (1.0f + (float)(q % 7)); cols[q] = colsf[q]; }
    // the reference's state: frag[] in the particles' order, a linking list through the members of each group in random order
    std::vector<float> frag(24 * cells);
    for (size_t i = 0; i < cells; i++) {
      size_t a = 0;
      pf_refresh_cell(b, pos[i], &a);
      for (int k = 0; k < 24; k++) frag[24 * i + k] = colsf[(size_t)k * ncell + a];
    }
    std::vector<PortGroup> groups(ngroups + 1);
    for (auto &g : groups) { g.point = -1; g.Mass = 0; for (int k = 0; k < 24; k++) g.v[k] = 7.0f; }
    std::vector<int> linking(cells), order(cells);
    for (size_t i = 0; i < cells; i++) { linking[i] = (int)i; order[i] = (int)i; }
    for (size_t i = cells; i > 1; i--) { const size_t j = rnd() % i; std::swap(order[i - 1], order[j]); }
    for (size_t q = 0; q < cells; q++) {
      const int i = order[q], g = gid[i];
      if (g < 2) continue;
      linking[i] = groups[g].point >= 0 ? groups[g].point : i;   // the new member goes in front
      groups[g].point = i; groups[g].Mass++;
    }
    port_group_velocities(ngroups, groups.data(), frag.data(), linking.data(), 2);
    for (const auto &sh : shapes) {
      std::vector<int> group(cells);
      std::vector<unsigned int> npart(cells);
      std::vector<double> sum(24 * cells);
      unsigned long long counted = 0;
      const unsigned long long G = emul_group_sums(cs.n, cs.x0, cs.nxl, cs.start, cs.len, cs.safe, cells, pos.data(), gid.data(), 2, cols.data(), sh[0], sh[1],
                                                   group.data(), npart.data(), sum.data(), &counted);
      unsigned long long seen = 0, present = 0;
      for (int g = 2; g <= ngroups; g++) present += groups[g].Mass > 0;
      if (G != present) { printf("MISMATCH: %llu groups, the port has %llu\n", G, present); return 1; }
      for (unsigned long long j = 0; j < G; j++) {
        const PortGroup &pg = groups[group[j]];
        if ((j && group[j] <= group[j - 1]) || npart[j] != (unsigned int)pg.Mass) { printf("MISMATCH at group %d\n", group[j]); return 1; }
        seen += npart[j];
        // sum |v| of the group, for the bound
        double sabs[24] = {0};
        int next = pg.point;
        for (int q = 0; q < pg.Mass; q++) { for (int k = 0; k < 24; k++) sabs[k] += fabs((double)frag[24 * (size_t)next + k]); next = linking[next]; }
        const double mm = pg.Mass, e = (mm - 1) * ldexp(1.0, -24), gamma = e / (1 - e);
        for (int k = 0; k < 24; k++) {
          const float mean = (float)(sum[24 * j + k] / mm);
          if (!(fabs((double)mean - (double)pg.v[k]) <= gamma * sabs[k] / mm + 2 * ldexp(1.0, -24) * fabs((double)mean))) {
            printf("MISMATCH: group %d column %d: %.9g, the port %.9g\n", group[j], k, mean, pg.v[k]);
            return 1;
          }
        }
      }
      if (seen != counted) { printf("MISMATCH: %llu particles in the groups, %llu counted\n", seen, counted); return 1; }
      printf("n %d box (%d %d %d)+(%d %d %d) unit %d x %d: groups %llu of %llu particles\n", cs.n, cs.start[0], cs.start[1], cs.start[2], cs.len[0], cs.len[1], cs.len[2],
             sh[0], sh[1], G, counted);
    }
  }
  // the production-size boxes: positions up to 2^32 - 1 from a sparse set, IDs up to 2^31 - 1, integer-valued columns (every sum is
  // exact); the last x-plane of the sub-box from a start that wraps in all three directions and the plane of position 2^31 from a
  // straight start, against sums kept per ID with the coordinates of keep_data_back (src/distribute.c:806-830)
  for (const LargeBox &lb : LARGE_BOXES) {
    const std::vector<unsigned int> pos = large_positions(lb.len, 200000, rnd);
    const size_t count = pos.size(), ncell = (size_t)lb.n * lb.n;
    std::vector<double> cols(24 * ncell);
    for (size_t q = 0; q < 24 * ncell; q++) cols[q] = (double)(((unsigned int)q * 2654435761u) >> 8);
    std::vector<int> gid(count);
    for (size_t i = 0; i < count; i++) {
      const unsigned int r = rnd() % 20;
      gid[i] = r < 5 ? 0x7FFFFFFF : r < 9 ? 2 : r < 12 ? 0x40003039 : r == 12 ? (int)(rnd() % 2) : (int)(2 + rnd() % 0x7FFFFFFD);
    }
    const int zero[3] = {0, 0, 0};
    unsigned long long ids[2], parts[2];
    for (int geo = 0; geo < 2; geo++) {
      const int *start = geo ? zero : lb.wrapped;
      const int x0 = geo ? large_mid_plane(lb.len) : (lb.wrapped[0] + lb.len[0] - 1) % lb.n;
      std::map<int, std::vector<double>> want;   // ID -> 24 sums and the count
      for (size_t iz = 0; iz < count; iz++) {
        const unsigned int I = pos[iz];
        unsigned int kbox = I % lb.len[2];
        const int kk = (int)(I / lb.len[2]);
        unsigned int jbox = kk % lb.len[1], ibox = kk / lb.len[1];
        ibox = (ibox + start[0] + lb.n) % lb.n; jbox = (jbox + start[1] + lb.n) % lb.n; kbox = (kbox + start[2] + lb.n) % lb.n;
        if (ibox != (unsigned int)x0 || gid[iz] < 2) continue;
        std::vector<double> &w = want[gid[iz]];
        if (w.empty()) w.assign(25, 0.0);
        for (int k = 0; k < 24; k++) w[k] += cols[(size_t)k * ncell + (size_t)kbox + (size_t)lb.n * jbox];
        w[24] += 1.0;
      }
      for (const auto &sh : shapes) {
        std::vector<int> group(count);
        std::vector<unsigned int> npart(count);
        std::vector<double> sum(24 * count);
        unsigned long long counted = 0;
        const unsigned long long G = emul_group_sums(lb.n, x0, 1, start, lb.len, lb.safe, count, pos.data(), gid.data(), 2, cols.data(), sh[0], sh[1], group.data(),
                                                     npart.data(), sum.data(), &counted);
        if (G != want.size() || !G) { printf("MISMATCH: large box %s: %llu IDs, the port has %zu\n", lb.name, G, want.size()); return 1; }
        unsigned long long j = 0, seen = 0;
        for (const auto &e : want) {   // (ascending ID)
          if (group[j] != e.first || (double)npart[j] != e.second[24]) { printf("MISMATCH: large box %s at ID %d\n", lb.name, e.first); return 1; }
          for (int k = 0; k < 24; k++)
            if (sum[24 * j + k] != e.second[k]) { printf("MISMATCH: large box %s: ID %d column %d\n", lb.name, e.first, k); return 1; }
          seen += npart[j];
          j++;
        }
        if (seen != counted) { printf("MISMATCH: large box %s: %llu particles summed, %llu counted\n", lb.name, seen, counted); return 1; }
        ids[geo] = G; parts[geo] = counted;
      }
    }
    printf("large box %s n %d (%d %d %d): %llu IDs of %llu particles on the last plane, %llu of %llu at 2^31\n", lb.name, lb.n, lb.len[0], lb.len[1], lb.len[2], ids[0],
           parts[0], ids[1], parts[1]);
  }
  return 0;
}
#endif
