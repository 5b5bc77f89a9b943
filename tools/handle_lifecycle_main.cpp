// handle_lifecycle_main.cpp -- the failure paths of the four create functions
// under AddressSanitizer and UndefinedBehaviorSanitizer, on a machine WITHOUT a
// GPU: every create gets as far as its first device call, fails there, and has
// to release what it made on the way (the handle, its design tables, a group's
// worker threads and the shards made before the failing one).  The library's
// translation units and this file go into one executable:
//
//   cd qpsk-modulator-demodulator_amd && mkdir -p _build/asan ../tools/bin
//   for f in csrc/*.hip csrc/*.cpp; do x=; b=$(basename ${f%.*}); \
//     case $f in *.cpp) x="-x c++";; *) b=${b}_dev;; esac; \
//     hipcc $x --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I../include -Icsrc \
//       -Xarch_host -fsanitize=address,undefined -c $f -o _build/asan/$b.o || break; done
//   hipcc -x c++ -std=c++17 -O1 -g -I../include -fsanitize=address,undefined \
//     -c ../tools/handle_lifecycle_main.cpp -o _build/asan/main.o
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined _build/asan/*.o -lpthread \
//     -o ../tools/bin/handle_lifecycle
//   ../tools/bin/handle_lifecycle
//
// (qpsk_ber and qpsk_channel are each one name in two files, .cpp and .hip: a
// .hip file's object carries _dev, so no two objects share a name.)
//
// It checks that each create returns QPSK_ERR_DEVICE, leaves *out null and a
// text in qpsk_last_error, and that every *_destroy(nullptr) returns what it
// always has.  A clean run ends with "0 failures" and no sanitizer report; the
// output is kept in profiles/handle_ownership_sanitizers.txt.  Not a pytest
// test; never run on a GPU machine (there the creates succeed and it fails).
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "qpsk_demod.h"

namespace {

int g_failures = 0;

void expect(const char *what, int rc, int want) {
    std::printf("%-28s status %d\n", what, rc);
    if (rc == want) return;
    ++g_failures;
    std::printf("FAIL: %s: status %d, expected %d (%s)\n", what, rc, want, qpsk_last_error());
}

// a create that must fail for want of a device
void expect_no_device(const char *what, int rc, const void *out) {
    const char *msg = qpsk_last_error();
    std::printf("%-28s status %d, out %s, \"%s\"\n", what, rc, out ? "SET" : "null", msg ? msg : "");
    if (rc == QPSK_ERR_DEVICE && !out && msg && *msg) return;
    ++g_failures;
    std::printf("FAIL: %s\n", what);
}

}  // namespace

int main() {
    qpsk_demod_params p;
    qpsk_demod_params_init(&p, 10000000, 1250000);
    p.max_samples_per_call = 4096;
    const uint8_t start[2] = {0xAA, 0x55}, end[2] = {0x55, 0xAA};
    const int32_t devices[2] = {0, 1};
    // twice over: what a failed create left behind must not trip the next one
    for (int round = 0; round < 2; ++round) {
        for (int fll = 0; fll < 2; ++fll) {
            p.enable_fll = fll;
            p.iq_balance = fll;
            qpsk_demod *h = reinterpret_cast<qpsk_demod *>(&p);   // any non-null value
            expect_no_device("qpsk_demod_create", qpsk_demod_create(&p, 8, &h), h);
        }
        qpsk_mod_params mp;
        qpsk_mod_params_init(&mp, 10000000, 1250000);
        qpsk_mod *m = reinterpret_cast<qpsk_mod *>(&p);
        expect_no_device("qpsk_mod_create", qpsk_mod_create(&mp, "0110100111", &m), m);
        qpsk_framer_dev *f = reinterpret_cast<qpsk_framer_dev *>(&p);
        expect_no_device("qpsk_framer_dev_create", qpsk_framer_dev_create(4, start, 2, end, 2, 4096, 0, &f), f);
        qpsk_demod_group *g = reinterpret_cast<qpsk_demod_group *>(&p);
        expect_no_device("qpsk_demod_group_create", qpsk_demod_group_create(&p, devices, 2, 8, &g), g);
    }
    expect("qpsk_demod_destroy(null)", qpsk_demod_destroy(nullptr), QPSK_OK);
    expect("qpsk_mod_destroy(null)", qpsk_mod_destroy(nullptr), QPSK_OK);
    expect("qpsk_framer_dev_destroy(null)", qpsk_framer_dev_destroy(nullptr), QPSK_OK);
    expect("qpsk_framer_destroy(null)", qpsk_framer_destroy(nullptr), QPSK_OK);
    expect("qpsk_demod_group_destroy(null)", qpsk_demod_group_destroy(nullptr), QPSK_OK);
    expect("qpsk_rx_destroy(null)", qpsk_rx_destroy(nullptr), QPSK_ERR_ARGUMENT_NULL);
    std::printf("handle lifecycle without a device: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
