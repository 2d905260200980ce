// setup_latch_check.cpp — the pair set-up's thread coordination (poppy_amd/csrc/setup_latch.h) alone, on the host, under a sanitizer:
//   clang++ -std=c++17 -O1 -g -fsanitize=thread            -pthread tools/setup_latch_check.cpp -o /tmp/latch_tsan && /tmp/latch_tsan
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread tools/setup_latch_check.cpp -o /tmp/latch_asan && /tmp/latch_asan
// Two threads play the two chains the way pair_begin.cpp's chain_of does, a few thousand rounds of each way a chain can leave.  A chain left
// waiting is a failure too: every case runs under an alarm.
#include "../poppy_amd/csrc/setup_latch.h"
#include <cstdio>
#include <cstring>
#include <thread>
#include <csignal>
#include <unistd.h>

using namespace poppy_hip;

enum Leave { kPublishes, kLeavesBeforeDetail };
enum Upload { kNone, kRecorded, kFails, kLeavesBeforeEvent };

struct Round {
    Details details; UploadKnown upload;
    double d[2] = {0, 0};             // plain, as in the set-up: written before the chain counts, read by the other after it has waited for 2
    bool saw_both[2] = {false, false}, upload_ok = false;
};

// chain i: (upload) -> detail -> publish -> wait for both -> read both details
static void chain(Round& r, int i, Leave leave, Upload up) {
    Publish publish{r.details};
    UploadExit upload_exit{r.upload, i == 1 && up != kNone};
    if (i == 1 && up == kLeavesBeforeEvent) return;
    if (i == 1 && up != kNone) { r.upload.known(up == kRecorded); if (up == kFails) return; }
    if (leave == kLeavesBeforeDetail) return;
    r.d[i] = 1.5 + i;
    publish.now();
    if (i == 0 && up != kNone && !(r.upload_ok = r.upload.wait())) return;      // the first chain, about to queue gabor2 behind the upload's event
    r.details.wait_for(2);
    r.saw_both[i] = r.d[0] == 1.5 && r.d[1] == 2.5;
}

static const char* g_case = "";
static void hung(int) {
    const char msg[] = "FAILED: a chain was left waiting in case: ";
    (void)!write(2, msg, sizeof msg - 1); (void)!write(2, g_case, strlen(g_case)); (void)!write(2, "\n", 1);
    _exit(2);
}

static int run(const char* name, int rounds, Leave l0, Leave l1, Upload up, bool want_both0, bool want_upload) {
    int bad = 0;
    g_case = name;
    alarm(60);                                                     // (a case takes well under a second; under the thread sanitizer a few)
    for (int k = 0; k < rounds; ++k) {
        Round r;
        if (up != kNone) r.upload.pending();
        std::thread other([&] { chain(r, 1, l1, up); });
        chain(r, 0, l0, up);
        other.join();
        if (r.saw_both[0] != want_both0 || r.upload_ok != want_upload) ++bad;
    }
    printf("%-52s %d rounds, %d wrong\n", name, rounds, bad);
    return bad;
}

int main() {
    const int n = 4000;
    int bad = 0;
    signal(SIGALRM, hung);
    bad += run("both chains publish", n, kPublishes, kPublishes, kNone, true, false);
    bad += run("both publish, staged upload recorded", n, kPublishes, kPublishes, kRecorded, true, true);
    bad += run("the second chain leaves before its detail", n, kPublishes, kLeavesBeforeDetail, kNone, false, false);
    bad += run("the first chain leaves before its detail", n, kLeavesBeforeDetail, kPublishes, kNone, false, false);
    bad += run("the upload fails: the waiter sees the failed state", n, kPublishes, kPublishes, kFails, false, false);
    bad += run("the uploader leaves before its event: failed state", n, kPublishes, kPublishes, kLeavesBeforeEvent, false, false);
    alarm(0);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
