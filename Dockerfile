# Two production images (VERDICT r1 #8), built from one Dockerfile:
#
#   --target control-plane  /app/{controller,admission,synchronizer} on debian:stable-slim
#                           with libssl + ca-certificates only, like the reference's runtime
#                           image (reference Dockerfile:20-28).  No ROCm, no test tools.
#   --target node-agent     /app/node-agent + the gfx950 diagnostics library, on a slim
#                           Ubuntu with only the ROCm user-space libraries the agent loads
#                           (libamd_smi, the HIP runtime and their dependencies), copied
#                           from the ROCm build stage by ldd closure.
#
# kube-lite, crdgen and bgc-certgen are development/test tools and ship in neither image
# (crdgen runs in CI: generate-crd.sh / check-crd-status.yml).
ARG ROCM_IMAGE=rocm/dev-ubuntu-22.04:7.2
ARG CP_BASE=debian:stable-slim
ARG NODE_BASE=ubuntu:22.04

# ---------------------------------------------------------------- control plane
FROM ${CP_BASE} AS build-cp
RUN apt-get update && apt-get install -y --no-install-recommends cmake ninja-build g++ libssl-dev && \
    rm -rf /var/lib/apt/lists/*
WORKDIR /src
COPY CMakeLists.txt ./
COPY native ./native
RUN cmake -S . -B build -G Ninja -DCMAKE_BUILD_TYPE=Release -DBGC_PYTHON=OFF && \
    ninja -C build controller admission synchronizer

FROM ${CP_BASE} AS control-plane
RUN apt-get update && apt-get install -y --no-install-recommends ca-certificates libssl3 && \
    rm -rf /var/lib/apt/lists/*
COPY --from=build-cp /src/bin/controller /src/bin/admission /src/bin/synchronizer /app/
# GLIBC_TUNABLES: deeper malloc tcache (+14% CR/s measured, profiles/archive/malloc_tunables_r1/).
# Only the thread cache (mallopt has no knob for it): arena count, heap growth and trimming
# are set by the binaries themselves, in one place (native/core/process.cc tune_malloc).
ENV GLIBC_TUNABLES=glibc.malloc.tcache_count=64:glibc.malloc.tcache_max=16384
USER 65532:65532

# ---------------------------------------------------------------- node agent (MI355X)
FROM ${ROCM_IMAGE} AS build-node
RUN apt-get update && apt-get install -y --no-install-recommends cmake ninja-build g++ libssl-dev && \
    rm -rf /var/lib/apt/lists/*
WORKDIR /src
COPY CMakeLists.txt ./
COPY native ./native
RUN cmake -S . -B build -G Ninja -DCMAKE_BUILD_TYPE=Release -DBGC_PYTHON=OFF && \
    ninja -C build node-agent && \
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared \
      -mllvm -amdgpu-mfma-vgpr-form=1 -Inative/gpu/hip native/gpu/hip/gpu_diag.hip native/gpu/hip/hbm.hip \
      native/gpu/hip/mfma.hip native/gpu/hip/lds.hip native/gpu/hip/cache.hip native/gpu/hip/valu.hip native/gpu/hip/atomic.hip native/gpu/hip/regfile.hip native/gpu/hip/xlane.hip native/gpu/hip/gemm_soak.hip \
      -o bin/libbgc_gpu_diag.so
# The agent dlopen()s libamd_smi and the diagnostics library (which links the HIP
# runtime): collect exactly those plus, to a fixpoint, their ROCm dependencies.  The same
# script runs in tests/gpu/test_node_image_closure.py, which runs the agent's diagnostics
# on an MI355X with only these libraries and checks nothing else came from /opt/rocm.
COPY tools/node_image_closure.sh ./tools/
RUN bash tools/node_image_closure.sh /rt /src/bin/libbgc_gpu_diag.so

FROM ${NODE_BASE} AS node-agent
RUN apt-get update && apt-get install -y --no-install-recommends ca-certificates libssl3 libdrm2 libdrm-amdgpu1 \
      libnuma1 libelf1 && rm -rf /var/lib/apt/lists/*
COPY --from=build-node /rt/ /opt/bgc/lib/
COPY --from=build-node /src/bin/node-agent /app/node-agent
ENV BGC_GPU_DIAG_LIB=/opt/bgc/lib/libbgc_gpu_diag.so \
    LD_LIBRARY_PATH=/opt/bgc/lib \
    GLIBC_TUNABLES=glibc.malloc.tcache_count=64:glibc.malloc.tcache_max=16384
# root: amdsmi reads /sys and the render/kfd nodes, the device plugin writes its socket
# into the kubelet's root-owned directory (chart: nodeAgent.securityContext)
