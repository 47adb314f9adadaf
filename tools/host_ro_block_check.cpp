// Stand-alone program for tools/host_ro_block_sanitize.sh: the two host entry points beside vdf_ro_hash_batch_block --
// vdf_nova_ro_block_constants and vdf_nova_ro_hash_batch_eval_ro -- at widths 2 and 25, both fields, on exact-size heap arrays (a
// read or write past one is the sanitizer's to see).  Values are held to vdf_nova_ro_hash_ro per message.  No device is touched.
#include <cstdio>
#include <cstring>
#include <vector>
#include "vdf_hip.h"
#include "vdf_nova.h"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "line %d: %s failed (%s)\n", __LINE__, #c, vdf_nova_last_error()); return 1; } } while (0)

int main() {
  int hashed = 0, refused = 0;
  for (int width : {2, 25}) {
    vdf_nova_ro_params ro;
    REQUIRE(vdf_nova_ro_preset(1, &ro) == VDF_OK);
    ro.width = width;
    const size_t rate = (size_t)width - 1, rounds = (size_t)(ro.full_rounds + ro.partial_rounds);
    for (int field : {VDF_FIELD_FP, VDF_FIELD_FQ}) {
      size_t counts[2] = {0, 0};
      REQUIRE(vdf_nova_ro_block_constants(&ro, field, nullptr, nullptr, counts) == VDF_OK);
      REQUIRE(counts[0] == rounds * width && counts[1] == (size_t)width * width);
      std::vector<vdf_fe> rc(counts[0]), mds(counts[1]);
      REQUIRE(vdf_nova_ro_block_constants(&ro, field, rc.data(), mds.data(), nullptr) == VDF_OK);
      REQUIRE(vdf_nova_ro_block_constants(&ro, field, rc.data(), nullptr, counts) == VDF_OK);
      REQUIRE(vdf_nova_ro_block_constants(&ro, field, nullptr, mds.data(), nullptr) == VDF_OK);
      const size_t n = 3;
      for (size_t len : {(size_t)0, (size_t)1, rate, rate + 1, 2 * rate + 1}) {
        std::vector<vdf_fe> xs(n * len), out(n), one(1);
        for (size_t k = 0; k < xs.size(); ++k) {          // small canonical elements; their Montgomery reading is as good as any
          memset(&xs[k], 0, sizeof(vdf_fe));
          const uint64_t v = 0x9E3779B97F4A7C15ull * (k + 1 + 1000 * len);
          memcpy(&xs[k], &v, 8);
        }
        for (int bits : {0, 1, 128, 250, 255}) {
          REQUIRE(vdf_nova_ro_hash_batch_eval_ro(&ro, field, 1, len ? xs.data() : nullptr, len, n, bits, out.data()) == VDF_OK);
          hashed += (int)n;
          if (bits) continue;
          for (size_t i = 0; i < n; ++i) {
            REQUIRE(vdf_nova_ro_hash_ro(&ro, field, 1, len ? xs.data() + i * len : nullptr, len, one.data()) == VDF_OK);
            REQUIRE(memcmp(&one[0], &out[i], sizeof(vdf_fe)) == 0);
          }
        }
        REQUIRE(vdf_nova_ro_hash_batch_eval_ro(&ro, field, 1, nullptr, len, 0, 250, nullptr) == VDF_OK);      // n = 0 touches nothing
      }
      std::vector<vdf_fe> xs(2 * 3), out(2);
      memset(xs.data(), 0, xs.size() * sizeof(vdf_fe));
      REQUIRE(vdf_nova_ro_hash_batch_eval_ro(&ro, 7, 1, xs.data(), 3, 2, 0, out.data()) == VDF_ERR_BAD_ARG);
      REQUIRE(vdf_nova_ro_hash_batch_eval_ro(&ro, field, 1, xs.data(), 3, 2, -1, out.data()) == VDF_ERR_BAD_ARG);
      REQUIRE(vdf_nova_ro_hash_batch_eval_ro(&ro, field, 1, xs.data(), 3, 2, 256, out.data()) == VDF_ERR_BAD_ARG);
      REQUIRE(vdf_nova_ro_hash_batch_eval_ro(&ro, field, 1, xs.data(), VDF_RO_HASH_MAX_LEN + 1, 2, 0, out.data()) == VDF_ERR_BAD_ARG);
      REQUIRE(vdf_nova_ro_hash_batch_eval_ro(&ro, field, 1, nullptr, 3, 2, 0, out.data()) == VDF_ERR_BAD_ARG);
      REQUIRE(vdf_nova_ro_hash_batch_eval_ro(&ro, field, 1, xs.data(), 3, 2, 0, nullptr) == VDF_ERR_BAD_ARG);
      vdf_nova_ro_params bad = ro;
      bad.width = VDF_RO_BLOCK_MAX_WIDTH + 1;
      REQUIRE(vdf_nova_ro_hash_batch_eval_ro(&bad, field, 1, xs.data(), 3, 2, 0, out.data()) == VDF_ERR_BAD_ARG);
      REQUIRE(vdf_nova_ro_block_constants(&bad, field, rc.data(), mds.data(), counts) == VDF_ERR_BAD_ARG);
      REQUIRE(vdf_nova_ro_block_constants(nullptr, field, rc.data(), mds.data(), counts) == VDF_ERR_BAD_ARG);
      REQUIRE(vdf_nova_ro_block_constants(&ro, 7, rc.data(), mds.data(), counts) == VDF_ERR_BAD_ARG);
      vdf_nova_ro_params dflt;
      REQUIRE(vdf_nova_ro_preset(0, &dflt) == VDF_OK);
      REQUIRE(vdf_nova_ro_block_constants(&dflt, field, rc.data(), mds.data(), counts) == VDF_ERR_BAD_ARG);
      refused += 11;
      // a null block is the default block's restatement
      std::vector<vdf_fe> a(2), b(2);
      REQUIRE(vdf_nova_ro_hash_batch_eval_ro(nullptr, field, 1, xs.data(), 3, 2, 250, a.data()) == VDF_OK);
      REQUIRE(vdf_nova_ro_hash_batch_eval(field, 1, xs.data(), 3, 2, 250, b.data()) == VDF_OK);
      REQUIRE(memcmp(a.data(), b.data(), 2 * sizeof(vdf_fe)) == 0);
    }
  }
  printf("host_ro_block_check: %d hashes at widths 2 and 25 in both fields, %d bad calls refused\n", hashed, refused);
  return 0;
}
