// Host side of the cooperative tile solve (tsolve.h: k_csolve): what every such launch of one engine shares, and the
// book-keeping between launches.
#pragma once
#include "host.h"
#include "tsolve.h"

namespace mmhn {

struct CoopState {
  DevArr<CoopCtl> ctl;              // queue heads + abort word
  DevArr<unsigned> flags[2];        // the flags of the tiles (value = epoch of the launch that finished the tile), one set per lane
                                    // that issues such launches (Lane::flags): two may be in flight together
  unsigned epoch = 0;
  int slot = 0;
  unsigned* h_abort = nullptr;      // the pinned host copy of the abort word
  unsigned* h_abort_dev = nullptr;  // device view of it
  bool used = false;                // an evaluation issued a cooperative launch since the last check_abort

  void init() {
    ctl.alloc(1);
    HIPCHECK(hipMemset(ctl.p, 0, sizeof(CoopCtl)));
    HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&h_abort), 64, hipHostMallocDefault));
    HIPCHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h_abort_dev), h_abort, 0));
    *h_abort = 0u;
  }
  void release() {
    if (h_abort) (void)hipHostFree(h_abort);
    h_abort = h_abort_dev = nullptr;
  }
  // what the next launch of nitems work items on lane L passes to the kernel, next to ctl.p and h_abort_dev
  struct Launch { unsigned* flags; unsigned epoch; int slot; };
  Launch begin_launch(const Lane& L, int nitems) {
    DevArr<unsigned>& f = flags[L.flags];
    if (f.n < (size_t)nitems) {
      HIPCHECK(hipStreamSynchronize(L.s));                // (a launch of this lane may still poll the old array)
      f.alloc((size_t)nitems + 1024);
      HIPCHECK(hipMemsetAsync(f.p, 0, f.n * sizeof(unsigned), L.s));
    }
    if (++epoch == 0u) {                                  // (wrapped: no stale flag may equal a future epoch)
      HIPCHECK(hipDeviceSynchronize());
      for (auto& g : flags) if (g.p) HIPCHECK(hipMemset(g.p, 0, g.n * sizeof(unsigned)));
      epoch = 1u;
    }
    slot = (slot + 1) & 3;
    used = true;
    return {f.p, epoch, L.flags * 4 + slot};
  }
  // a spin of a cooperative launch timed out (tsolve.h): the results of the evaluation are garbage - fail the call, and put
  // the words back so that the engine stays usable.  Call after the stream has been synchronised.
  void check_abort() {
    if (!used) return;
    used = false;
    if (*h_abort == 0u) return;
    *h_abort = 0u;
    (void)hipMemset(ctl.p, 0, sizeof(CoopCtl));
    throw Fail{"cooperative tile solve: a wait for another workgroup's tile timed out (results discarded)"};
  }
};

}  // namespace mmhn
