// Test infrastructure (tests/test_vocab_tables_host.py): build_vocab_tables
// (lddl_amd/csrc/tok_tables.h) built for the host with g++ under
// AddressSanitizer + UBSan, run over one vocab.txt.  Prints "key=value" facts
// about the tables: where the keys landed, whether a host restatement of the
// WordPiece kernel's bucket probe (vhash, two slots, next bucket, pool compare
// past 24 bytes; tokenize_split.hip wp_kernel) finds every key again with the
// id the last such line has, whether every key's Bloom and extension bits are
// set, and whether rinfo / rpool give every entry back.  The Bloom and
// extension bits are checked as the builder defines them (every 4-, 8-, ..
// 24-byte prefix shorter than the key), not as wp_kernel walks them: that the
// kernel's chain (TOK5_EXT / TOK5_GROUP) agrees with them shows only on the
// GPU, in tests/test_tokenize_vocab_gpu.py over the 'ext' vocabulary.
//   host_vocab_tables VOCAB [--dump]     (--dump: every entry in hex, by id)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "tok_tables.h"

using namespace lddl;

struct Hit { int id; uint32_t dist; int slot; };

// the probe of wp_kernel for a candidate of len bytes with the "##" flag cont
static Hit probe(const VocabTables& V, const uint8_t* s, uint32_t len, uint32_t cont) {
  uint32_t d[VKEY_DW] = {0, 0, 0, 0, 0, 0};
  memcpy(d, s, len < 24 ? len : 24);
  const uint32_t want = (len << 16) | (cont << 24) | 0x80000000u;
  uint32_t b = vhash(d, len, cont) & V.vt_mask;
  for (uint32_t dist = 0; dist <= V.vt_mask; ++dist, b = (b + 1) & V.vt_mask) {
    bool empty = false;
    for (int sl = 0; sl < 2; ++sl) {
      const uint32_t* q = &V.vt[((size_t)b * 2 + sl) * 8];
      if (!(q[6] & 0x80000000u)) { empty = true; continue; }
      if ((q[6] & 0xFFFF0000u) != want || memcmp(q, d, sizeof d) != 0) continue;
      if (len > 24 && memcmp(&V.pool[q[7] + 24], s + 24, len - 24) != 0) continue;
      return Hit{(int)(q[6] & 0xFFFFu), dist, sl};
    }
    if (empty) break;  // an empty slot ends the probe sequence
  }
  return Hit{-1, 0, 0};
}

static bool bloom_has(const VocabTables& V, uint32_t k) {
  const uint32_t bb = vbloom_bits(k);
  return (V.vbloom[vbloom_word(k)] & bb) == bb;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: host_vocab_tables VOCAB [--dump]\n");
    return 2;
  }
  VocabTables V;
  std::string err;
  const int rc = build_vocab_tables(argv[1], V, err);
  printf("rc=%d\n", rc);
  printf("eformat=%d\n", rc == LDDL_EFORMAT ? 1 : 0);
  if (rc) {
    printf("err=%s\n", err.c_str());
    return 0;
  }
  const size_t n = V.vocab.size();
  std::map<std::pair<uint32_t, std::string>, int> last;  // (cont, key) -> the last line that holds it
  for (size_t i = 0; i < n; ++i) {
    const std::string& w = V.vocab[i];
    const uint32_t cont = (w.size() >= 2 && w[0] == '#' && w[1] == '#') ? 1u : 0u;
    last[{cont, w.substr(2 * cont)}] = (int)i;
  }
  uint32_t max_probe = 0, long_keys = 0, whole_off_slot0 = 0, not_found = 0, bloom_missing = 0, ext_missing = 0,
           render_bad = 0, keys = 0, mb[2] = {0, 0};
  for (const auto& kv : last) {
    const uint32_t cont = kv.first.first;
    const std::string& k = kv.first.second;
    const uint32_t len = (uint32_t)k.size();
    if (len == 0) continue;  // "" and "##": no word or piece is empty
    ++keys;
    if (len > 24) ++long_keys;
    if (len > mb[cont]) mb[cont] = len;
    const Hit h = probe(V, reinterpret_cast<const uint8_t*>(k.data()), len, cont);
    if (h.id != kv.second) { ++not_found; continue; }
    if (h.dist > max_probe) max_probe = h.dist;
    if (!cont && (h.dist != 0 || h.slot != 0)) ++whole_off_slot0;
    uint32_t d[VKEY_DW] = {0, 0, 0, 0, 0, 0};
    memcpy(d, k.data(), len < 24 ? len : 24);
    if (!bloom_has(V, vbkey_of(d, len, cont))) ++bloom_missing;
    uint32_t hp = VSEED;
    for (uint32_t j = 0; j < (uint32_t)VKEY_DW && 4 * (j + 1) < len; ++j) {
      hp = vmix(hp, d[j]);
      if (!bloom_has(V, vbkey_ext(hp, 4 * (j + 1), cont))) ++ext_missing;
    }
  }
  // a key that is no line of the file is not found
  {
    const std::string no = "\x01no such key\x02";
    if (probe(V, reinterpret_cast<const uint8_t*>(no.data()), (uint32_t)no.size(), 0).id != -1) ++not_found;
  }
  for (size_t i = 0; i < n; ++i) {
    const std::string& w = V.vocab[i];
    const uint32_t off = V.rinfo[i] >> 8, len = V.rinfo[i] & 0xFFu;
    if (len != w.size() || (size_t)off + len > V.rpool.size() || memcmp(&V.rpool[off], w.data(), len) != 0) ++render_bad;
  }
  printf("n=%zu\nkeys=%u\nmaxb0=%u\nmaxb1=%u\nkey_maxb0=%u\nkey_maxb1=%u\n", n, keys, V.maxb[0], V.maxb[1], mb[0], mb[1]);
  printf("special=%u,%u,%u,%u,%u\n", V.special[0], V.special[1], V.special[2], V.special[3], V.special[4]);
  printf("long_keys=%u\nmax_probe=%u\nwhole_off_slot0=%u\nnot_found=%u\nbloom_missing=%u\next_missing=%u\nrender_bad=%u\n",
         long_keys, max_probe, whole_off_slot0, not_found, bloom_missing, ext_missing, render_bad);
  if (argc > 2 && strcmp(argv[2], "--dump") == 0)
    for (size_t i = 0; i < n; ++i) {
      printf("entry=%zu:", i);
      for (unsigned char ch : V.vocab[i]) printf("%02x", ch);
      printf("\n");
    }
  return 0;
}
