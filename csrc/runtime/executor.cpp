// trtlab_amd — graph-captured executor (MI355X-native replacement for the
// reference's TensorRT workspace/enqueueV2 path, trtlab/tensorrt/src/
// workspace.cc:21-75: bindings + activation scratch + warm-up + cudaGraph
// capture + replay — here with our own op plan over CDNA4 kernels).
#include <cstring>

#include "runtime.h"
#include "../kernels/launchers.h"

namespace trtlab {

Engine::Engine(int device, const void* weights, size_t weight_bytes,
               size_t arena_bytes, std::vector<OpDesc> ops,
               std::vector<BindingDesc> inputs,
               std::vector<BindingDesc> outputs, bool managed_weights)
    : device_(device),
      weight_bytes_(weight_bytes),
      managed_weights_(managed_weights),
      arena_bytes_(arena_bytes),
      ops_(std::move(ops)),
      inputs_(std::move(inputs)),
      outputs_(std::move(outputs)) {
  if (inputs_.empty() || outputs_.empty())
    throw std::runtime_error("Engine needs >=1 input and >=1 output binding");
  TRT_HIP_CHECK(hipSetDevice(device_));
  size_t wb = weight_bytes_ ? weight_bytes_ : 256;
  if (managed_weights_) {
    // reference ManagedRuntime: weights in managed memory, advised
    // read-mostly and prefetched so steady-state reads hit HBM
    TRT_HIP_CHECK(hipMallocManaged(&weights_, wb));
    if (weight_bytes_) {
      std::memcpy(weights_, weights, weight_bytes_);
      (void)hipMemAdvise(weights_, wb, hipMemAdviseSetReadMostly, device_);
      (void)hipMemPrefetchAsync(weights_, wb, device_, 0);
    }
  } else {
    weights_ = device_malloc(wb, device_);
    if (weight_bytes_)
      TRT_HIP_CHECK(
          hipMemcpy(weights_, weights, weight_bytes_, hipMemcpyHostToDevice));
  }
  zero_page_ = device_malloc(256, device_);
  TRT_HIP_CHECK(hipMemset(zero_page_, 0, 256));
  // Split-K slab workspace: sized to the worst op in the plan.
  for (const OpDesc& op : ops_) {
    if (op.kind == kConv2d)
      scratch_bytes_ = std::max(
          scratch_bytes_,
          conv_scratch_bytes(op.Nb, op.H, op.W, op.C, op.Cout, op.KH, op.KW,
                             op.sh, op.sw, op.ph, op.pw));
    else if (op.kind == kGemmBt)
      scratch_bytes_ =
          std::max(scratch_bytes_, gemm_scratch_bytes(op.M, op.N, op.K));
  }
  TRT_HIP_CHECK(hipDeviceSynchronize());
}

Engine::~Engine() {
  if (managed_weights_)
    (void)hipFree(weights_);
  else
    device_free(weights_, weight_bytes_ ? weight_bytes_ : 256);
  device_free(zero_page_, 256);
}

void Engine::upload_weights(const void* src, size_t bytes) {
  if (bytes > weight_bytes_) throw std::runtime_error("upload_weights: too large");
  TRT_HIP_CHECK(hipSetDevice(device_));
  TRT_HIP_CHECK(hipMemcpy(weights_, src, bytes,
                          managed_weights_ ? hipMemcpyDefault
                                           : hipMemcpyHostToDevice));
  if (managed_weights_)
    (void)hipMemPrefetchAsync(weights_, bytes, device_, 0);
}

ExecutionContext::ExecutionContext(std::shared_ptr<Engine> engine,
                                   uintptr_t external_arena)
    : eng_(std::move(engine)) {
  TRT_HIP_CHECK(hipSetDevice(eng_->device()));
  if (external_arena) {
    arena_ = (char*)external_arena;  // caller-owned (shared DeviceArena)
    owns_arena_ = false;
  } else {
    arena_ = (char*)device_malloc(eng_->arena_bytes(), eng_->device());
  }
  if (eng_->scratch_bytes())
    scratch_ = (char*)device_malloc(eng_->scratch_bytes(), eng_->device());
  // Carve one pinned slab per direction into per-binding regions, each
  // 256-B aligned (reference Buffers::CreateBindings carving pattern).
  for (const BindingDesc& b : eng_->inputs()) {
    in_hoff_.push_back(h_in_bytes_);
    h_in_bytes_ += round_up(b.bytes, 256);
  }
  for (const BindingDesc& b : eng_->outputs()) {
    out_hoff_.push_back(h_out_bytes_);
    h_out_bytes_ += round_up(b.bytes, 256);
  }
  h_in_ = (char*)pinned_malloc(h_in_bytes_);
  h_out_ = (char*)pinned_malloc(h_out_bytes_);
  TRT_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  // fork/join resources: one side stream + 2 events per forked op + a
  // private split-K slab so forked convs never race the main chain's
  int nfork = 0;
  for (const OpDesc& op : eng_->ops()) nfork += op.fork ? 1 : 0;
  if (nfork) {
    TRT_HIP_CHECK(hipStreamCreateWithFlags(&side_, hipStreamNonBlocking));
    fork_ev_.resize(2 * nfork);
    for (auto& e : fork_ev_)
      TRT_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (eng_->scratch_bytes())
      scratch2_ = (char*)device_malloc(eng_->scratch_bytes(), eng_->device());
  }
}

ExecutionContext::~ExecutionContext() {
  for (auto& e : ev_)
    if (e) hipEventDestroy(e);
  for (auto& e : fork_ev_) hipEventDestroy(e);
  if (graph_exec_) hipGraphExecDestroy(graph_exec_);
  if (graph_) hipGraphDestroy(graph_);
  if (side_) hipStreamDestroy(side_);
  if (scratch2_) device_free(scratch2_, eng_->scratch_bytes());
  hipStreamDestroy(stream_);
  if (owns_arena_) device_free(arena_, eng_->arena_bytes());
  if (scratch_) device_free(scratch_, eng_->scratch_bytes());
  pinned_free(h_in_, h_in_bytes_);
  pinned_free(h_out_, h_out_bytes_);
}

void ExecutionContext::enqueue_all(hipStream_t s) {
  const char* wb = eng_->weights();
  char* ar = arena_;
  auto A = [&](int64_t off) -> void* { return off < 0 ? nullptr : ar + off; };
  auto Wp = [&](int64_t off) -> const void* {
    return off < 0 ? nullptr : wb + off;
  };
  auto Fp = [&](int64_t off) -> const float* {
    return off < 0 ? nullptr : (const float*)(wb + off);
  };

  if (timing_ && !ev_[0])
    for (auto& e : ev_) TRT_HIP_CHECK(hipEventCreate(&e));
  if (timing_) TRT_HIP_CHECK(hipEventRecord(ev_[0], s));
  const auto& ins = eng_->inputs();
  for (size_t i = 0; i < ins.size(); ++i)
    TRT_HIP_CHECK(hipMemcpyAsync(ar + ins[i].off, h_in_ + in_hoff_[i],
                                 ins[i].bytes, hipMemcpyHostToDevice, s));
  if (timing_) TRT_HIP_CHECK(hipEventRecord(ev_[1], s));

  // fork/join dual-stream schedule: forked ops (downsample convs) run on
  // side_ overlapping the main chain; the consuming op waits on the
  // branch's event. Event record/wait inside stream capture become graph
  // dependencies, so the replayed hipGraph keeps the fork/join shape.
  int evi = 0;
  hipEvent_t pending_join = nullptr;
  for (const OpDesc& op : eng_->ops()) {
    hipStream_t os = s;
    if (op.join && pending_join) {
      TRT_HIP_CHECK(hipStreamWaitEvent(s, pending_join, 0));
      pending_join = nullptr;
    }
    if (op.fork && side_) {
      hipEvent_t ef = fork_ev_[evi++];
      TRT_HIP_CHECK(hipEventRecord(ef, s));
      TRT_HIP_CHECK(hipStreamWaitEvent(side_, ef, 0));
      os = side_;
    }
    switch (op.kind) {
      case kConv2d:
        launch_conv2d(op.dtype, A(op.in_off), Wp(op.w_off), A(op.out_off),
                      Fp(op.scale_off), Fp(op.bias_off), A(op.in2_off),
                      eng_->zero_page(), op.Nb, op.H, op.W, op.C, op.Cout,
                      op.KH, op.KW, op.sh, op.sw, op.ph, op.pw, op.epi, os,
                      op.tile, op.fork ? scratch2_ : scratch_, op.res_scale);
        break;
      case kConst:
        // device constant: blob -> arena slot (captured in the graph)
        TRT_HIP_CHECK(hipMemcpyAsync(A(op.out_off), Wp(op.w_off),
                                     (size_t)op.n_elems,
                                     hipMemcpyDeviceToDevice, os));
        break;
      case kView:
        break;  // arena alias — out_off == in_off, nothing to launch
      case kChAffine:
        launch_channel_affine(op.dtype, A(op.in_off), A(op.out_off),
                              Fp(op.scale_off), Fp(op.bias_off),
                              op.n_elems, op.C, op.epi != 0, os);
        break;
      case kBtail:
        // fused bottleneck tail: W1 at w_off, W2 at w2_off; the fp32
        // scale/bias blobs hold [s1 | s2] / [b1 | b2] (s2 at + C floats)
        launch_bottleneck_tail(op.dtype, A(op.in_off), Wp(op.w_off),
                               Wp(op.w2_off), A(op.out_off),
                               Fp(op.scale_off), Fp(op.bias_off),
                               Fp(op.scale_off) + op.C,
                               Fp(op.bias_off) + op.C, A(op.in2_off),
                               eng_->zero_page(), op.Nb, op.H, op.W, op.C,
                               op.Cout, os);
        break;
      case kGemmBt:
        launch_gemm_bt(op.dtype, A(op.in_off), Wp(op.w_off), A(op.out_off),
                       Fp(op.scale_off), Fp(op.bias_off), A(op.in2_off),
                       op.res_scale, op.M, op.N, op.K, op.K /*lda*/,
                       op.K /*ldb*/, op.N /*ldc*/, op.epi, os, op.tile,
                       scratch_, op.q_scale /*post-epilogue out scale*/);
        break;
      case kMaxPool:
        launch_maxpool2d(op.dtype, A(op.in_off), A(op.out_off), op.Nb, op.H,
                         op.W, op.C, op.KH, op.KW, op.sh, op.sw, op.ph, op.pw,
                         os);
        break;
      case kAvgPool:
        launch_avgpool2d(op.dtype, A(op.in_off), A(op.out_off), op.Nb, op.H,
                         op.W, op.C, op.KH, op.KW, op.sh, op.sw, op.ph,
                         op.pw, os);
        break;
      case kGAvgPool:
        launch_gavgpool(op.dtype, A(op.in_off), A(op.out_off), op.Nb, op.HW,
                        op.C, os);
        break;
      case kSoftmax:
        launch_softmax_rows(op.dtype, A(op.in_off), A(op.out_off), op.M, op.N,
                            op.N, os);
        break;
      case kLayerNorm:
        // epi 0: out2 (optional) = fused fp8 copy at q_scale.
        // epi 4/8: producer-fused MX — out2 = codes, out3 = e8m0 scales.
        launch_layernorm(op.dtype, A(op.in_off), Fp(op.scale_off),
                         Fp(op.bias_off), A(op.out_off), op.M, op.N, op.N,
                         op.eps, os,
                         op.epi ? nullptr : A(op.out2_off), op.q_scale,
                         op.epi ? A(op.out2_off) : nullptr, A(op.out3_off),
                         op.epi);
        break;
      case kAddLayerNorm:
        launch_add_layernorm(op.dtype, A(op.in_off), A(op.in2_off),
                             Fp(op.scale_off), Fp(op.bias_off), A(op.out_off),
                             nullptr /*sum_out*/, op.M, op.N, op.N, op.eps, os,
                             op.epi ? nullptr : A(op.out2_off), op.q_scale,
                             op.epi ? A(op.out2_off) : nullptr,
                             A(op.out3_off), op.epi);
        break;
      case kElementwise:
        launch_elementwise(op.dtype, op.epi, A(op.in_off), A(op.in2_off),
                           A(op.out_off), op.n_elems, os);
        break;
      case kChannelPad:
        launch_channel_pad(op.dtype, A(op.in_off), A(op.out_off), op.n_elems,
                           op.C, op.Cout, os);
        break;
      case kAttention:
        // epi = output dtype flag (3 -> fused fp8 out at 1/q_scale)
        launch_attention(op.dtype, A(op.in_off), A(op.out_off), op.B, op.S,
                         op.NH, op.HD, op.att_scale, os, op.epi,
                         op.q_scale != 0.f && op.epi == 3
                             ? 1.0f / op.q_scale
                             : 1.0f,
                         A(op.in2_off) /*seqlens or null*/, op.causal,
                         op.NKV);
        break;
      case kSeqLens:
        // op.epi carries pad_id
        launch_seqlens(A(op.in_off), A(op.out_off), op.B, op.S, op.epi, os);
        break;
      case kQuantMx4:
        // out = fp4 codes, out2 = e8m0 block scales
        launch_quantize_mxfp4(A(op.in_off), A(op.out_off), A(op.out2_off),
                              op.M, op.K, os);
        break;
      case kGemmMx4:
        // A/Sa = quantized activations (arena), B/Sb = weights (blob)
        launch_gemm_mxfp4(A(op.in_off), Wp(op.w_off), A(op.in2_off),
                          Wp(op.w2_off), A(op.out_off), op.M, op.N, op.K, os,
                          0 /*fp16 out*/, op.epi, Fp(op.scale_off),
                          Fp(op.bias_off));
        break;
      case kQuantMx8:
        launch_quantize_mxfp8(A(op.in_off), A(op.out_off), A(op.out2_off),
                              op.M, op.K, os);
        break;
      case kGemmMx8:
        launch_gemm_mxfp8(A(op.in_off), Wp(op.w_off), A(op.in2_off),
                          Wp(op.w2_off), A(op.out_off), op.M, op.N, op.K, os,
                          0 /*fp16 out*/, op.epi, Fp(op.scale_off),
                          Fp(op.bias_off));
        break;
      case kQuantize:
        // op.epi carries the target format (0 = int8, 1 = fp8 e4m3)
        launch_quantize(A(op.in_off), A(op.out_off), op.n_elems, op.q_scale,
                        os, op.epi);
        break;
      case kDequant:
        launch_dequant(A(op.in_off), A(op.out_off), op.n_elems, op.q_scale,
                       os, op.epi);
        break;
      case kEmbedding:
        // tables live in the weight blob as fp16: tok at w_off, pos at
        // scale_off, optional seg at bias_off; optional segids at in2_off.
        launch_embedding(op.dtype, A(op.in_off), Wp(op.w_off),
                         Wp(op.scale_off), Wp(op.bias_off), A(op.in2_off),
                         A(op.out_off), op.M, op.S, op.N, os);
        break;
      case kRMSNorm:
        launch_rmsnorm(op.dtype, A(op.in_off), Fp(op.scale_off),
                       A(op.out_off), op.M, op.N, op.N, op.eps, os);
        break;
      case kSiluMul:
        launch_silu_mul(op.dtype, A(op.in_off), A(op.in2_off), A(op.out_off),
                        op.n_elems, os);
        break;
      case kRope:
        // in-place on the (arena-aliased) qkv buffer; eps carries theta
        launch_rope(op.dtype, A(op.out_off), nullptr, op.M, op.S, op.NH,
                    op.HD, op.eps, os, 0, op.NKV);
        break;
      case kClip:
        // res_scale = min bound, q_scale = max bound
        launch_clip(op.dtype, A(op.in_off), A(op.out_off), op.n_elems,
                    op.res_scale, op.q_scale, os);
        break;
      case kTranspose2D:
        launch_transpose2d(op.dtype, A(op.in_off), A(op.out_off), op.M, op.N,
                           os);
        break;
      case kCopy2D:
        // epi = destination column offset; Cout = destination row stride
        launch_copy2d(op.dtype, A(op.in_off), A(op.out_off), op.M, op.C,
                      op.Cout, op.epi, os);
        break;
      default:
        throw std::runtime_error("unknown op kind");
    }
    if (op.fork && side_) {  // branch completion event for the join
      hipEvent_t ej = fork_ev_[evi++];
      TRT_HIP_CHECK(hipEventRecord(ej, side_));
      pending_join = ej;
    }
  }
  if (pending_join)  // safety: never leave a branch dangling past the D2H
    TRT_HIP_CHECK(hipStreamWaitEvent(s, pending_join, 0));

  if (timing_) TRT_HIP_CHECK(hipEventRecord(ev_[2], s));
  const auto& outs = eng_->outputs();
  for (size_t i = 0; i < outs.size(); ++i)
    TRT_HIP_CHECK(hipMemcpyAsync(h_out_ + out_hoff_[i], ar + outs[i].off,
                                 outs[i].bytes, hipMemcpyDeviceToHost, s));
  if (timing_) TRT_HIP_CHECK(hipEventRecord(ev_[3], s));
}

std::array<float, 3> ExecutionContext::stage_times_ms() const {
  std::array<float, 3> out = {0.f, 0.f, 0.f};
  if (!ev_[0]) return out;
  for (int i = 0; i < 3; ++i)
    TRT_HIP_CHECK(hipEventElapsedTime(&out[i], ev_[i], ev_[i + 1]));
  return out;
}

void ExecutionContext::capture() {
  TRT_HIP_CHECK(hipSetDevice(eng_->device()));
  // warm-up (module loading, autotune state) before capture — reference
  // workspace.cc:47 does one enqueueV2 before cudaStreamBeginCapture.
  enqueue_all(stream_);
  TRT_HIP_CHECK(hipStreamSynchronize(stream_));
  TRT_HIP_CHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeRelaxed));
  enqueue_all(stream_);
  TRT_HIP_CHECK(hipStreamEndCapture(stream_, &graph_));
  TRT_HIP_CHECK(hipGraphInstantiate(&graph_exec_, graph_, nullptr, nullptr, 0));
  captured_ = true;
}

void ExecutionContext::launch() {
  if (captured_) {
    TRT_HIP_CHECK(hipGraphLaunch(graph_exec_, stream_));
  } else {
    enqueue_all(stream_);
  }
}

void ExecutionContext::synchronize() {
  TRT_HIP_CHECK(hipStreamSynchronize(stream_));
}

bool ExecutionContext::ready() {
  hipError_t e = hipStreamQuery(stream_);
  if (e == hipSuccess) return true;
  if (e == hipErrorNotReady) return false;
  TRT_HIP_CHECK(e);
  return false;
}

}  // namespace trtlab
