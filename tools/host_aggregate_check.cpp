// Stand-alone program for tools/host_aggregate_sanitize.sh: vdf_nova_aggregate_fold_instances (the verifier's transcript and folds of
// "vdf-aggregate-v1", host only) on the inputs of tests/golden/aggregate.json and on damaged copies of them.  No device is touched.
//
//   host_aggregate_check <file>
// <file>: one case per line, hex without spaces (written by the script from the golden file):
//   <side> <digest 32 B> <count> <count x 160 B instances> <(count - 1) x 32 B points or "-"> <expected folded instance 160 B>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "vdf_nova.h"

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return out;
}

static int fold(int side, const std::vector<uint8_t>& digest, size_t count, const std::vector<uint8_t>& inst, const std::vector<uint8_t>& tt,
                vdf_wire_instance* acc, std::vector<vdf_fe>* r) {
  // exact-size heap copies: a read past either array is the sanitizer's to see
  std::vector<vdf_wire_instance> in(count);
  if (count) memcpy(in.data(), inst.data(), count * sizeof(vdf_wire_instance));
  std::vector<uint8_t> pts(tt);
  r->assign(count > 1 ? count - 1 : 0, vdf_fe{});
  return vdf_nova_aggregate_fold_instances(VDF_FIELD_FQ, side, digest.data(), count, in.data(),
                                           count > 1 ? reinterpret_cast<const uint8_t(*)[32]>(pts.data()) : nullptr, acc, r->empty() ? nullptr : r->data());
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: host_aggregate_check <cases file>\n"); return 2; }
  std::ifstream f(argv[1]);
  std::string line;
  int cases = 0, refused = 0;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    int side; size_t count; std::string d, i, t, e;
    if (!(ss >> side >> d >> count >> i >> t >> e)) continue;
    const std::vector<uint8_t> digest = unhex(d), inst = unhex(i), tt = unhex(t), want = unhex(e);
    if (digest.size() != 32 || inst.size() != 160 * count || tt.size() != 32 * (count - 1) || want.size() != 160) { fprintf(stderr, "bad case line\n"); return 2; }
    vdf_wire_instance acc;
    std::vector<vdf_fe> r;
    if (fold(side, digest, count, inst, tt, &acc, &r) != VDF_OK) { fprintf(stderr, "case %d: %s\n", cases, vdf_nova_last_error()); return 1; }
    if (memcmp(&acc, want.data(), 160) != 0) { fprintf(stderr, "case %d: folded instance differs from the golden one\n", cases); return 1; }
    ++cases;
    // damaged copies: every prefix of the instances (a shorter count), an element out of range, bytes that are no point
    for (size_t k = 1; k < count; ++k)
      if (fold(side, digest, k, inst, std::vector<uint8_t>(tt.begin(), tt.begin() + 32 * (k - 1)), &acc, &r) != VDF_OK) return 1;
    std::vector<uint8_t> bad = inst;
    memset(&bad[64], 0xff, 32);                                       // u >= m
    if (fold(side, digest, count, bad, tt, &acc, &r) != VDF_ERR_NONCANONICAL) return 1;
    ++refused;
    bad = inst;
    memset(&bad[0], 0, 32); bad[31] = 0x80;                            // the identity with the parity bit set
    if (fold(side, digest, count, bad, tt, &acc, &r) != VDF_ERR_NONCANONICAL) return 1;
    ++refused;
    if (fold(side, digest, 0, inst, tt, &acc, &r) != VDF_ERR_BAD_ARG) return 1;
    if (vdf_nova_aggregate_fold_instances(VDF_FIELD_FQ, side, digest.data(), count, nullptr, nullptr, &acc, nullptr) != VDF_ERR_BAD_ARG) return 1;
    refused += 2;
  }
  if (cases == 0) { fprintf(stderr, "no case read\n"); return 2; }
  printf("host_aggregate_check: %d golden folds reproduced, %d damaged inputs refused\n", cases, refused);
  return 0;
}
