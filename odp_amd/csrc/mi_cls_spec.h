// mi_cls_spec.h -- the compile manager of the program-specialised kernels
// (mi_cls_spec.cpp): source text in, a kernel loaded on a device out.
#pragma once
#include <hip/hip_runtime_api.h>

#include <memory>
#include <string>

struct SpecCode;   // one compiled (or compiling) specialised kernel

// The specialisation of (hipRTC program, instantiation name): the cached
// one, or a new one queued for the compile thread (a request still waiting
// to start is dropped for it).  Null when the cache is full: the generic
// kernels run.
std::shared_ptr<SpecCode> mi_spec_request(const std::string &src, const std::string &inst);

// Compile on the calling thread, outside the cache (mi_cls_spec_compile):
// 0, or -ENOEXEC when the compiler failed.
int mi_spec_compile_now(const std::string &src, const std::string &inst);

// The kernel of `sc` on `device`, loaded there on first use (wait: block
// until the compilation ends).  False: still compiling.  True: *fn is the
// kernel, or null when it failed, was dropped or does not load.
bool mi_spec_function(SpecCode &sc, int device, bool wait, hipFunction_t *fn);
