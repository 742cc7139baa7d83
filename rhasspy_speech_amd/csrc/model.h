// Host-side model description: everything the hot path reads from disk, parsed into plain
// structs (no Kaldi types).  File/line citations refer to /root/reference/kaldi/src.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "kaldi_io.h"
#include "recurrent_walk.h"

namespace rs {

// ---------------------------------------------------------------- feature options
// feat/feature-window.h:40-116, feat/mel-computations.h:43-75, feat/feature-mfcc.h:40-80
struct MfccOptions {
  float samp_freq = 16000, frame_shift_ms = 10, frame_length_ms = 25, dither = 1.0f, preemph = 0.97f;
  bool remove_dc = true, round_pow2 = true, snip_edges = true;
  bool allow_downsample = false, allow_upsample = false;   // feature-window.h:95-107: the reference then resamples (LinearResample); the library refuses such input
  std::string window_type = "povey";
  float blackman_coeff = 0.42f;
  int num_bins = 23;
  float low_freq = 20, high_freq = 0, vtln_low = 100, vtln_high = -500;
  int num_ceps = 13;
  bool use_energy = true, raw_energy = true, htk_compat = false;
  float energy_floor = 0, cepstral_lifter = 22;
  int WindowShift() const { return (int)(samp_freq * 0.001f * frame_shift_ms); }
  int WindowSize() const { return (int)(samp_freq * 0.001f * frame_length_ms); }
  int PaddedWindowSize() const;
};

// feat/feature-fbank.h:41-81: the frame and mel options of MfccOptions (num_ceps and cepstral_lifter are not options here) with
// this type's own defaults, and the two switches only it has
struct FbankOptions : MfccOptions {
  bool use_log_fbank = true, use_power = true;
  FbankOptions() { use_energy = false; }
  int Dim() const { return num_bins + (use_energy ? 1 : 0); }      // feature-fbank.h:93-95
};

// Tables the base-feature kernel needs, computed once on the host with the reference's float/double
// expression order (feature-window.cc:113-125, mel-computations.cc:33-142,253-259,
// matrix-functions.cc:592-608).  For a log-mel filterbank model (fbank = true) nceps is the row's width, num-mel-bins (+ 1 with
// the energy), opts holds the FbankOptions' shared part, and there is no DCT and no lifter.
struct MfccTables {
  MfccOptions opts;
  int win = 0, shift = 0, padded = 0, nbins = 0, nceps = 0;
  bool fbank = false, use_log_fbank = true, use_power = true;
  int energy_col = -1, mel_col0 = 0;      // fbank: the energy's column (-1: none) and the first mel column
  std::vector<float> window;      // win
  std::vector<int> mel_offset;    // nbins: first FFT bin of each filter
  std::vector<int> mel_len;       // nbins
  std::vector<int> mel_start;     // nbins: offset into mel_weights
  std::vector<float> mel_weights; // concatenated
  std::vector<float> dct;         // nceps x nbins
  std::vector<float> lifter;      // nceps (1.0 if no liftering)
  float log_energy_floor = 0;
};
void ReadMfccOptions(const std::string &conf_path, MfccOptions *o);
void BuildMfccTables(const MfccOptions &o, MfccTables *t);
void ReadFbankOptions(const std::string &conf_path, FbankOptions *o);
void BuildFbankTables(const FbankOptions &o, MfccTables *t);
int NumFrames(long num_samples, const MfccOptions &o);  // feature-window.cc:42-87 (snip_edges only)

// feat/online-feature.h:200-260
struct CmvnOptions {
  int cmn_window = 600, speaker_frames = 600, global_frames = 200;
  bool normalize_mean = true, normalize_variance = false;
};

// online2/online-ivector-feature.h:60-160 + the files it names
struct IvectorExtractor {
  bool present = false;
  // config
  int ivector_period = 10, num_gselect = 5, num_cg_iters = 15;
  float min_post = 0.025f, posterior_scale = 0.1f, max_count = 0.0f, max_remembered_frames = 1000;
  bool use_most_recent_ivector = true, greedy = false, online_cmvn_iextractor = false;
  int splice_left = 0, splice_right = 0;
  CmvnOptions cmvn;
  // data
  MatF lda;                 // D_lda x (C*nsplice [+1])
  MatD global_cmvn;         // 2 x (C+1)
  std::vector<float> gconsts, weights;   // UBM (gconsts recomputed like DiagGmm::ComputeGconsts)
  MatF means_invvars, inv_vars;          // G x D_lda
  std::vector<MatD> M;                   // G x (D_lda x D_iv)
  std::vector<std::vector<double>> sigma_inv;  // G x packed(D_lda)
  double prior_offset = 0;
  // derived (ivector-extractor.cc:182-218)
  std::vector<double> U;            // G x D_iv(D_iv+1)/2
  std::vector<double> sigma_inv_M;  // G x D_lda x D_iv
  int feat_dim() const { return lda.rows; }
  int ivector_dim() const { return M.empty() ? 0 : M[0].cols; }
  int num_gauss() const { return (int)M.size(); }
  void ComputeDerived();
};

// online2/online-nnet2-feature-pipeline.h (OnlineNnet2FeaturePipelineConfig / Info)
struct FeatureConfig {
  std::string feature_type = "mfcc";
  MfccTables mfcc;
  bool use_cmvn = false;   // --cmvn-config on the nnet input branch
  CmvnOptions cmvn;
  MatD global_cmvn;
  IvectorExtractor ie;
  // Decoder / decodable options found in online.conf.  The reference registers them on the parser that reads --config
  // (online2-wav-nnet3-latgen-faster.cc:131-137, online2-cli-nnet3-decode-faster.cc:73-78), so they take effect there unless the
  // command line repeats them (util/parse-options.cc:328-345: the config file is read first).  Model::Model applies them.
  std::vector<std::pair<std::string, std::string>> decoder_conf;
  std::vector<std::pair<std::string, std::string>> endpoint_conf;      // the --endpoint.* lines, in file order (Model::EndpointOpts)
  std::string conf_path;
};
void ReadFeatureConfig(const std::string &online_conf, FeatureConfig *fc);

// ---------------------------------------------------------------- transition model
// hmm/hmm-topology.cc:39-161, hmm/transition-model.cc:144-177,394-420
struct TransitionModel {
  int num_pdfs = 0;
  std::vector<int32_t> id2pdf;     // index = transition-id (0 unused)
  std::vector<int32_t> id2phone;
  // for the lattice tools of the rescoring path (lat/lattice-functions.cc:423-441, hmm/hmm-utils.cc:1065-1084):
  std::vector<int32_t> id2hmm_state;   // TransitionIdToHmmState
  std::vector<char> id2self_loop;      // IsSelfLoop
  std::vector<float> log_prob;         // GetTransitionLogProb
  std::vector<float> non_self_loop_log_prob;   // GetNonSelfLoopLogProb of the transition-id's transition-state
  // for graph construction (hmm/hmm-utils.cc:30-150,470-560): the topology and the tuple table themselves
  struct HmmState { int fwd = -1, self = -1; std::vector<std::pair<int, float>> trans; };   // pdf classes, (destination, prob)
  struct Tuple { int phone, hmm_state, fwd, self; };
  std::vector<std::vector<HmmState>> topo_entries;
  std::vector<int32_t> phone2entry;            // index = phone, -1 = no topology
  std::vector<Tuple> tuples;                   // transition-state k (1-based) = tuples[k - 1]
  std::vector<int32_t> tstate_first_tid;       // per transition-state (1-based; [0] unused): its first transition-id
  std::vector<int32_t> id2tstate;              // TransitionIdToTransitionState
  std::vector<int32_t> self_loop_of_id;        // per transition-id: SelfLoopOf(its transition-state), 0 = none
  int NumTransitionIds() const { return (int)id2pdf.size() - 1; }
  int TupleToTransitionState(int phone, int hmm_state, int fwd, int self) const;     // 0 = not found
  int NumPdfClasses(int phone) const;
  void Read(KaldiReader &r);
};

// ---------------------------------------------------------------- nnet3
// A parsed component blob.  `f` holds every basic value that followed each token, `m`/`v`/`iv` the
// matrices / vectors / integer vectors, `flags` the bare tokens.
struct Component {
  std::string type;
  std::map<std::string, std::vector<double>> f;      // basic values read as floating point
  std::map<std::string, std::vector<int64_t>> i;     // the same values read as integers (binary files do not say which)
  int Int(const std::string &k, int idx = 0) const { return (int)i.at(k).at(idx); }
  std::map<std::string, MatF> m;
  std::map<std::string, std::vector<float>> v;
  std::map<std::string, std::vector<int32_t>> iv;
  std::map<std::string, bool> b;
  bool Has(const std::string &k) const { return f.count(k) || m.count(k) || v.count(k) || iv.count(k) || b.count(k); }
};

// One term of a descriptor sum: scale * node[t + offset]; `const_t` = ReplaceIndex(x, t, 0) / Round (per-utterance row).
struct DescTerm {
  int node = -1;
  int offset = 0;
  float scale = 1.0f;
  bool const_t = false;
  bool optional = false;   // inside IfDefined(): the recurrent connections of a block are written that way
  bool konst = false;      // Const(value, dim): no node (node = -1), `scale` holds the value; only the (1 - z_t) of a composed GRU block
};
// Append(part0, part1, ...) where each part is a Sum of terms of equal dim.
struct DescPart {
  std::vector<DescTerm> terms;
  int dim = 0;
};
struct Descriptor {
  std::vector<DescPart> parts;
  int dim = 0;
};

struct NnetNode {
  enum Kind { kInput, kComponent, kOutput, kDimRange } kind = kInput;
  std::string name;
  int dim = 0;
  int component = -1;      // kComponent
  Descriptor input;        // kComponent / kOutput
  int range_node = -1, range_offset = 0;   // kDimRange
};

// Executable layer plan.  Every op produces one buffer with rows t in [-lext, T+rext) per utterance.
struct GemmSegment {
  int src_buf = -1;     // buffer index; -1 = iVector input (one row per utterance/chunk)
  int src_col = 0;      // first column inside the source buffer
  int ncols = 0;        // K extent of this segment
  int offset = 0;       // time offset
  int w_col = 0;        // first column in the weight matrix
};
struct EltStage {
  enum Kind { kRelu, kScaleOffset, kLogSoftmax, kNormalize, kScale } kind = kRelu;
  std::vector<float> scale, offset;   // kScaleOffset (BatchNorm test mode, ScaleAndOffset, PerElementScale...)
  float alpha = 1.0f;                 // kScale / kNormalize target_rms
};
struct SumTerm { int src_buf; int src_col; int offset; float scale; };
// TimeHeightConvolutionComponent (nnet3/convolution.h:125-208): rows are frames, columns (height, filter) with the filter
// fastest; weight column = offset index * filters_in + filter, offsets in (time, height) order.
struct ConvGeom {
  int filters_in = 0, filters_out = 0, height_in = 0, height_out = 0, height_sub = 1;
  std::vector<std::pair<int, int>> offsets;   // (time, height), sorted
  std::vector<int> time_offsets;              // the distinct time offsets, ascending: LayerOp::terms[i] reads the rows of time_offsets[i]
  int K() const { return (int)offsets.size() * filters_in; }
};
// A recurrent block: what nnet3's fast-lstmp-layer / fast-lstm-layer emit (xconfig/lstm.py), recognised as a unit (Nnet::Compile).
// With s_c, s_r the state rows (zero where the chain has not started), d the delay, per row t:
//   gates = pre[t] + W_r s_r[t - d]                                   pre = W_x x + b, a kGemm op over all rows
//   (c, m) = LstmNonlinearity(gates, s_c[t - d]; params)              cu-math.cc:445-486
//   rp = W_rp m + b_rp                                                with a projection
//   s_c[t] = scale c,  s_r[t] = scale rp[0:rec] (or scale m)          BackpropTruncationComponent::Propagate
struct LstmBlock {
  int in_dim = 0, cell = 0, rec = 0, nonrec = 0;   // rec / nonrec: the projection's dims, 0 / 0 without one (the recurrent input is then m)
  int delay = 0;                  // frames towards the past, 1 .. kLstmMaxDelay
  float scale = 1.0f;
  bool dropout_mask = false;      // use-dropout=true with its DropoutMaskComponent node: all ones in test mode
  // the composed form (LayerOp::kLstmp, below): `scale` is the <Scale> of the truncation component `c`, scale_r that of `r`;
  // dropout: the shared DropoutComponent behind i, f and o is present (a copy in test mode); cm_buf holds [sc | m]
  bool composed = false;
  float scale_r = 1.0f;
  bool dropout = false;
  // the bottleneck form (LayerOp::kLstmb, below): bottleneck > 0, rec = nonrec = 0; W_r is W_all_a's recurrent columns
  // (bottleneck x cell), W_b is W_all_b (4 cell x bottleneck), so_scale / so_offset W_all_b_so's vectors (4 cell, EnsureNonzero
  // applied), self_scale the Scale() on the recurrent input; pre_buf is bottleneck wide, st_buf holds [sc | sm]
  int bottleneck = 0;
  float self_scale = 1.0f;
  MatF W_b;
  std::vector<float> so_scale, so_offset;
  MatF W_r;                       // 4 cell x RecDim(): W_all's recurrent columns
  MatF params;                    // 3 x cell: w_ic, w_fc, w_oc
  MatF W_rp;                      // (rec + nonrec) x cell
  std::vector<float> b_rp;
  // buffers: pre-activations (4 cell), the nonlinearity's output [c | m], rp (-1 without a projection), the state [s_c | s_r]
  int pre_buf = -1, cm_buf = -1, rp_buf = -1, st_buf = -1;
  // rows: a call that starts an utterance walks t from -lext of these buffers (the first t at which x is computable from the input
  // the first chunk requests); an advance that continues a stream re-enters at t0 - need_lext with the state it parked
  int need_lext = 0;
  bool proj() const { return rec > 0; }
  int RecDim() const { return rec > 0 ? rec : cell; }
  int OutDim() const { return rec > 0 ? rec + nonrec : cell; }
  int StateDim() const { return bottleneck > 0 ? 2 * cell : cell + RecDim(); }      // a parked state row: [s_c | s_r], behind a bottleneck [sc | sm]
};
// The same cell spelled out as separate components: what nnet3's lstmp-layer / lstmp-batchnorm-layer / lstm-layer emit
// (xconfig/lstm.py: XconfigLstmpLayer, XconfigLstmLayer), recognised as a unit and held in an LstmBlock with composed = true.  Four
// affines over Append(x, IfDefined(Offset(r_t, -d))) stacked in gate order i, f, c(g), o (pre = W_x x + b a kGemm op, W_r their
// recurrent columns), three NaturalGradientPerElementScaleComponent peepholes (params), Sigmoid / Tanh nodes, three
// ElementwiseProductComponents, two truncation components.  With sc, sr the outputs of c_t and r_t, per row t, every product and
// sum a rounding of its own:
//   i = Sigmoid((pre_i + W_ri sr[t - d]) + w_ic . sc[t - d]),  f likewise,  g = Tanh(pre_g + W_rg sr[t - d])
//   sc[t] = scale (f . sc[t - d] + i . g);  o = Sigmoid((pre_o + W_ro sr[t - d]) + w_oc . sc[t]);  m = o . Tanh(sc[t])
//   rp = W_rp m + b_rp,  sr[t] = scale_r rp[0:rec]     or, without a projection,     sr[t] = scale_r m
// The cell with its affine factorised through a bottleneck: what nnet3's lstmb-layer emits (xconfig/lstm.py: XconfigLstmbLayer),
// recognised as a unit and held in an LstmBlock with bottleneck > 0.  Two LinearComponents (no bias) and a ScaleAndOffsetComponent in
// front of the LstmNonlinearityComponent, one BackpropTruncationComponent over [c | m], Scale(self_scale, m_trunc) on the recurrent
// input.  With sc, sm the state rows, per row t, every line a rounding of its own:
//   b = pre_b[t] + W_a,m sm[t - d]          pre_b = W_a,x x, a kGemm op over all rows
//   g = W_b b;  g' = g * so_scale;  g' = g' + so_offset                     ScaleAndOffsetComponent::PropagateInternal
//   (c, m) = LstmNonlinearity(g', sc[t - d]; params)
//   sc[t] = scale c;  sm[t] = self_scale (scale m)                          the second product only where self_scale is not 1

// A recurrent block of the output-gate projected GRU: what nnet3's fast-opgru-layer / fast-norm-opgru-layer emit (xconfig/gru.py),
// recognised as a unit (Nnet::Compile).  With s the recurrent state (scaled), c the cell state (read back unscaled), zero where the
// chain has not started, d the delay, per row t:
//   z = Sigmoid(pre_z[t] + W_z,s s[t - d]),  o = Sigmoid(pre_o[t] + W_o,s s[t - d])     pre = [W_z,x; W_o,x; W_hpart] x + b, a kGemm op
//   h = Tanh(pre_h[t] + w_h . c[t - d]);  c = h - z . h + z . c[t - d]                   OutputGruNonlinearityComponent::Propagate
//   y = W_y (c . o) + b_y                                                                ElementwiseProductComponent, affine
//   s[t] = scale y[0:rec]   or, norm,   scale Normalize(y[0:rec])                        BackpropTruncationComponent::Propagate
struct GruBlock {
  int in_dim = 0, cell = 0, rec = 0, nonrec = 0;
  int delay = 0;                  // frames towards the past, 1 .. kLstmMaxDelay
  float scale = 1.0f;
  bool norm = false;              // fast-norm-opgru-layer: a NormalizeComponent between y[0:rec] and the truncation component
  float target_rms = 1.0f;        // its <TargetRms>
  bool dropout = false;           // the norm variant's shared DropoutComponent behind the sigmoids: a copy in test mode
  // the composed form (opgru-layer / norm-opgru-layer: the cell spelled out as Sigmoid / Tanh / ElementwiseProduct / NoOp nodes, w_h a
  // NaturalGradientPerElementScaleComponent's <Params>): the same operands and buffers, walked by nnet_gruc.hip in that form's order,
  //   c = fl(fl(h . fl(1 - z)) + fl(c[t - d] . z))
  bool composed = false;
  MatF W_s;                       // 2 cell x rec: the recurrent columns of W_z over those of W_o
  std::vector<float> w_h;         // cell
  MatF W_y;                       // (rec + nonrec) x cell
  std::vector<float> b_y;
  // buffers: pre-activations [z | o | hpart] (3 cell), the nonlinearity's output [h | c], y (rec + nonrec), the state s (rec)
  int pre_buf = -1, hc_buf = -1, y_buf = -1, s_buf = -1;
  int need_lext = 0;              // as LstmBlock::need_lext
  int StateDim() const { return cell + rec; }      // a parked state row: [c | s]
};

// A recurrent block of the (projected) GRU with a reset gate: what nnet3's fast-pgru-layer / fast-norm-pgru-layer / fast-gru-layer
// emit (xconfig/gru.py) around a GruNonlinearityComponent, recognised as a unit (Nnet::Compile).  With s the recurrent state
// (scaled), c the cell state (read back unscaled), zero where the chain has not started, d the delay, R = RecDim(), per row t:
//   z = Sigmoid(pre_z[t] + W_z,s s[t - d])  (cell),  r = Sigmoid(pre_r[t] + W_r,s s[t - d])  (R)     pre = [W_z,x; W_r,x; W_hpart] x + b, a kGemm op
//   sdotr = r . s[t - d];  h = Tanh(pre_h[t] + W_h sdotr);  c = h - z . h + z . c[t - d]             GruNonlinearityComponent::Propagate
//   y = W_y c + b_y;  s[t] = scale y[0:rec]   or, norm,   scale Normalize(y[0:rec])                  affine, BackpropTruncationComponent
// Without a projection (fast-gru-layer: rec = nonrec = 0) R = cell, there is no W_y, s[t] = scale c, and c[t - d] IS s[t - d].
struct PgruBlock {
  int in_dim = 0, cell = 0, rec = 0, nonrec = 0;   // rec / nonrec: W_y's dims, 0 / 0 without a projection
  int delay = 0;                  // frames towards the past, 1 .. kLstmMaxDelay
  float scale = 1.0f;
  bool norm = false;              // fast-norm-pgru-layer: a NormalizeComponent between y[0:rec] and the truncation component
  float target_rms = 1.0f;        // its <TargetRms>
  bool dropout = false;           // the norm variant's two DropoutComponents behind the sigmoids: copies in test mode
  // the composed form (pgru-layer / norm-pgru-layer / gru-layer: the cell spelled out as Sigmoid / Tanh / ElementwiseProduct / NoOp
  // nodes, W_h the recurrent columns of the affine W_h.UW): the same operands and buffers, walked by nnet_gruc.hip in that form's
  // order, c = fl(fl(h . fl(1 - z)) + fl(c[t - d] . z))
  bool composed = false;
  MatF W_zs;                      // cell x RecDim(): the recurrent columns of W_z
  MatF W_rs;                      // RecDim() x RecDim(): those of W_r
  MatF W_h;                       // cell x RecDim(): the nonlinearity's <w_h>
  MatF W_y;                       // (rec + nonrec) x cell; empty without a projection
  std::vector<float> b_y;
  // buffers: pre-activations [z | r | hpart] (2 cell + RecDim()), the nonlinearity's output [h | c], y (rec + nonrec; -1 without a
  // projection), the state s (RecDim())
  int pre_buf = -1, hc_buf = -1, y_buf = -1, s_buf = -1;
  int need_lext = 0;              // as LstmBlock::need_lext
  bool proj() const { return rec > 0; }
  int RecDim() const { return rec > 0 ? rec : cell; }
  int OutDim() const { return rec > 0 ? rec + nonrec : cell; }
  int StateDim() const { return rec > 0 ? cell + rec : cell; }      // a parked state row: [c | s], without a projection [s]
};

// RestrictedAttentionComponent (nnet3/nnet-attention-component.h, attention.h): an input row is `heads` blocks of
// [key(K) | value(V) | query(K + C)], C = left + 1 + right; an output row is `heads` blocks of [value(V) | c(C) if output_context].
// Per frame t and head, o = 0 .. C-1:  b[o] = key_scale <query_key(t), key(t + (o - left) stride)> + query_context(t)[o],
// c = softmax(b), value_out = sum_o c[o] value(t + (o - left) stride).
struct AttentionGeom {
  int heads = 0, key_dim = 0, value_dim = 0, left = 0, right = 0, stride = 1;
  bool output_context = true;
  float key_scale = 1.0f;
  int Context() const { return left + 1 + right; }
  int InDimPerHead() const { return 2 * key_dim + value_dim + Context(); }
  int OutDimPerHead() const { return value_dim + (output_context ? Context() : 0); }
  int InDim() const { return heads * InDimPerHead(); }
  int OutDim() const { return heads * OutDimPerHead(); }
  int TimeOffset(int o) const { return (o - left) * stride; }
};

struct LayerOp {
  // kConv: out = stages(bias + conv(terms)); kGather: out[:, i] = part(gather_part[i])[:, gather_col[i]] (PermuteComponent over an Append)
  // kLstm: the serial part of a recurrent block (lstm); out_buf = lstm.cm_buf.  kGru: the same of a GRU block (gru); out_buf = gru.hc_buf
  // kPgru: the same of a block around a GruNonlinearityComponent (pgru); out_buf = pgru.hc_buf
  // kLstmp: the same of an LSTM block in its composed form (lstm, with lstm.composed); out_buf = lstm.cm_buf
  // kLstmb: the same of an LSTM block in its bottleneck form (lstm, with lstm.bottleneck > 0); out_buf = lstm.cm_buf
  // kAttention: out = attention(terms[0]), no fused stage (the result matrix of the op is the component's output): one term, the source; the rows it reads are terms[0].offset + attention.TimeOffset(o)
  enum Kind { kGemm, kEltwise, kConv, kGather, kLstm, kGru, kAttention, kPgru, kLstmp, kLstmb } kind = kGemm;
  std::string name;
  int out_buf = -1, out_dim = 0;
  // kGemm
  std::vector<GemmSegment> segs;
  MatF W;                       // out_dim x K (K = sum of segment widths, Kaldi column order)
  std::vector<float> bias;      // may be empty
  // a two-term Sum() folded into this GEMM (Nnet::Compile: the residual of a factorised TDNN layer, Sum(Scale(0.66, previous), this)):
  // out = stages(W x + b) + res_scale * res_buf[t], computed with the float operations of the elementwise op it replaces
  int res_buf = -1;
  float res_scale = 1.0f;
  // kEltwise: out = stages(sum_i scale_i * src_i[t+o_i])
  // kConv: one term per distinct time offset (the same source, offset = descriptor offset + time offset; scale 1), W and bias as
  // for kGemm.  kGather: one term per Append part, in order.
  std::vector<SumTerm> terms;
  std::vector<EltStage> stages; // applied after the gemm/sum, in order
  ConvGeom conv;                           // kConv
  std::vector<int> gather_part, gather_col;   // kGather, per output column: the term and the column inside it
  LstmBlock lstm;                             // kLstm, kLstmp, kLstmb
  GruBlock gru;                               // kGru
  AttentionGeom attention;                    // kAttention
  PgruBlock pgru;                             // kPgru
};
struct BufferInfo {
  int dim = 0, lext = 0, rext = 0;   // rows cover t in [-lext, T + rext)
  bool is_input = false;             // the MFCC ("input") buffer
  int stride = 1;                    // > 1 (--frame-subsampling-factor): only the rows t = 0 mod stride are read by anybody
};

struct Nnet {
  std::vector<NnetNode> nodes;
  std::vector<std::string> component_names;
  std::vector<Component> components;
  std::vector<float> priors;
  int input_dim = 0, ivector_dim = 0, output_dim = 0;
  // plan
  std::vector<LayerOp> ops;
  std::vector<BufferInfo> bufs;
  int input_buf = -1, output_buf = -1;
  int left_context = 0, right_context = 0;
  bool recurrent = false;      // has at least one recurrent block (kLstm, kLstmp, kLstmb, kGru or kPgru op)
  // What the reference's binaries do to the network before the first frame (nnet3_setup.h): the network is the one
  // CollapseModel leaves behind, and rand() has been called `setup_rand_calls` times (the dither seeds follow from that).
  long setup_rand_calls = 0;
  bool setup_rand_certain = true;
  std::string setup_rand_uncertain_why;
  void Read(KaldiReader &r, int frames_per_chunk = 24, int extra_left_context_initial = 0, int frame_subsampling_factor = 1);
  void ParseNodes(const std::vector<std::string> &config_lines);   // nodes (and the dims) from config lines and the components read
  void Compile();   // builds ops/bufs for the "output" node
  void SetSubsampling(int factor);   // fills BufferInfo::stride for outputs wanted at t = 0, factor, 2 factor, ...
  int FindNode(const std::string &name) const;
};

// The geometry of a parsed TimeHeightConvolutionComponent, checked as the reference checks it at load (and refused where its
// required time offsets are fewer than its time offsets)
ConvGeom ReadConvGeom(const Component &c, const std::string &name);

// The geometry of a parsed RestrictedAttentionComponent, checked as RestrictedAttentionComponent::Check() checks it; refused
// (naming `node` where it is known) where a required input count is smaller than the input count: zero padding in time
AttentionGeom ReadAttentionGeom(const Component &c, const std::string &name, const std::string &node = std::string());

// <NumComponents> ... </Nnet3> (nnet-nnet.cc:608-621)
void ReadNnetComponents(KaldiReader &r, std::vector<std::string> *names, std::vector<Component> *comps);

struct AcousticModel {
  TransitionModel trans;
  Nnet nnet;
  void Read(const std::string &final_mdl, int frames_per_chunk = 24, int extra_left_context_initial = 0, int frame_subsampling_factor = 1);
};

// ---------------------------------------------------------------- HCLG
// fstext/kaldi-fst-io.cc:51-91; openfst lib/fst.cc:58-82; const-fst.h:192-232; vector-fst.h
struct FstArc { int32_t ilabel, olabel; float weight; int32_t nextstate; };
struct Hclg {
  int32_t start = -1;
  std::vector<float> final_cost;     // per state (+inf = non-final)
  std::vector<uint32_t> arc_begin;   // per state, size n+1
  std::vector<uint32_t> num_ieps;    // per state: number of input-epsilon arcs (sorted first)
  std::vector<FstArc> arcs;          // ilabel-sorted within each state if the file was
  int num_states() const { return (int)final_cost.size(); }
  void Read(const std::string &path);
};

std::vector<std::string> ReadWordsTxt(const std::string &path);

}  // namespace rs
