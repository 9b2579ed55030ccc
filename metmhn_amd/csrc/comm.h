// RCCL, opened at run time: the communicator of an engine whose cohort is sharded over several GPUs.
#pragma once
#include <rccl/rccl.h>                 // types only: the library is opened at run time by mmhn_comm_init
#include <dlfcn.h>

#include <string>

#include "host.h"

namespace mmhn {

// RCCL entry points, resolved on first use (a single-GPU process never loads the library).  "librccl.so.1" is the
// soname both ROCm and the PyTorch wheel ship: inside a torch.distributed process this is the copy already loaded.
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static Rccl& rccl() {
  static Rccl r;
  if (r.lib) return r;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* lib = nullptr;
  for (const char* nm : names) if ((lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL))) break;
  if (!lib) throw Fail{std::string("cannot load RCCL: ") + dlerror()};
  auto sym = [&](const char* nm) {
    void* f = dlsym(lib, nm);
    if (!f) throw Fail{std::string("RCCL symbol missing: ") + nm};
    return f;
  };
  r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
  r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
  r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
  r.CommCount = reinterpret_cast<decltype(r.CommCount)>(sym("ncclCommCount"));
  r.CommUserRank = reinterpret_cast<decltype(r.CommUserRank)>(sym("ncclCommUserRank"));
  r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(sym("ncclAllReduce"));
  r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
  r.lib = lib;
  return r;
}
#define RCCLCHECK(expr)                                                                          \
  do {                                                                                           \
    ncclResult_t r_ = (expr);                                                                    \
    if (r_ != ncclSuccess) throw Fail{std::string(#expr) + ": " + rccl().GetErrorString(r_)};    \
  } while (0)

}  // namespace mmhn
