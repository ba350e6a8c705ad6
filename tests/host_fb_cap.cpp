// fb_list_cap (lddl_amd/csrc/tokenize.h) on the host: prints the capacity in
// sentence ranges for every "seg_tiles n_sent" pair of the command line, one
// per line (tests/test_fb_cap_host.py compares them with a model of the scan's
// windows).
#include <cstdio>
#include <cstdlib>

#include "tokenize.h"

int main(int argc, char** argv) {
  if (argc < 3 || (argc - 1) % 2 != 0) {
    fprintf(stderr, "usage: %s seg_tiles n_sent [seg_tiles n_sent ...]\n", argv[0]);
    return 2;
  }
  for (int i = 1; i + 1 < argc; i += 2) {
    char *e0 = nullptr, *e1 = nullptr;
    const long long seg = strtoll(argv[i], &e0, 10), n_sent = strtoll(argv[i + 1], &e1, 10);
    if (*e0 || *e1 || seg < 1 || n_sent < 0) {
      fprintf(stderr, "bad pair: %s %s\n", argv[i], argv[i + 1]);
      return 2;
    }
    printf("%lld\n", (long long)lddl::fb_list_cap(seg, n_sent));
  }
  return 0;
}
