/* rhasspy_speech_hip.h -- C ABI of librhasspy_speech_hip.so
 *
 * Drop-in boundary for the transcribe hot path of rhasspy/rhasspy-speech.  The reference crosses a
 * *process* boundary here: rhasspy_speech/transcribe_wav.py:45-75 pipes
 *     online2-wav-nnet3-latgen-faster | lattice-to-nbest | nbest-to-linear
 * and rhasspy_speech/transcribe_stream.py:53-99 feeds s16le PCM to online2-cli-nnet3-decode-faster and
 * then runs the same two lattice tools.  Each entry point below names the piece of that contract it
 * replaces.  Plain C types only; every call returns 0 on success and a negative status on failure, with
 * the message available from rs_last_error() (the reference's convention: non-zero exit status + stderr
 * text, rhasspy_speech/tools.py:138-145).  Handles are opaque.  The caller owns every input buffer; the
 * library owns results until rs_result_free().
 *
 * There is NO CPU fallback: model parsing runs on the host, every compute entry point needs an MI355X
 * (gfx950) device and fails with RS_ERR_DEVICE otherwise.
 */
#ifndef RHASSPY_SPEECH_HIP_H_
#define RHASSPY_SPEECH_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_OK 0
#define RS_ERR_ARG -1     /* bad argument */
#define RS_ERR_MODEL -2   /* model/graph/config file could not be read (Kaldi's KALDI_ERR paths) */
#define RS_ERR_DEVICE -3  /* no usable HIP device / HIP runtime error */
#define RS_ERR_DECODE -4  /* decoding failed (e.g. no frames) */

typedef struct rs_model rs_model;
typedef struct rs_result rs_result;
typedef struct rs_stream rs_stream;

/* Options = the command-line flags the reference passes (transcribe_wav.py:46-55,
 * transcribe_stream.py:55-60) plus the Kaldi defaults it relies on
 * (decoder/lattice-faster-decoder.h:38-92, nnet3/decodable-simple-looped.h:50-60). */
/* rs_decode_opts is the command line of the reference's binaries.  The reference registers the decoder's and the decodable's
 * options on the parser that reads --config=online.conf (online2-wav-nnet3-latgen-faster.cc:131-137,
 * online2-cli-nnet3-decode-faster.cc:73-78) and ParseOptions reads the config file FIRST, the command line overriding it
 * (util/parse-options.cc:328-345).  Same here: a field left at RS_OPT_UNSET takes online.conf's value if the file sets the option
 * and the reference's default otherwise; any other value wins over online.conf.  rs_default_opts() sets what rhasspy passes on
 * the command line (transcribe_wav.py:46-55: --max-active --lattice-beam --acoustic-scale --beam) and leaves the rest unset.
 * Options of online.conf the kernels cannot honour (--extra-left-context-initial != 0,
 * --prune-interval != 25, --determinize-lattice=false, --online=true, --do-endpointing=true) fail the model load. */
#define RS_OPT_UNSET (-1)
typedef struct rs_decode_opts {
  float beam;                  /* --beam            (24.0 as rhasspy runs it; reference default 16.0) */
  int32_t max_active;          /* --max-active      (7000 as rhasspy runs it; reference default INT32_MAX) */
  int32_t min_active;          /* --min-active      (unset; reference default 200) */
  float lattice_beam;          /* --lattice-beam    (8.0 as rhasspy runs it; reference default 10.0) */
  float beam_delta;            /* --beam-delta      (unset; reference default 0.5) */
  float acoustic_scale;        /* --acoustic-scale of the decodable (1.0 as rhasspy runs it; reference default 0.1) */
  int32_t frames_per_chunk;    /* --frames-per-chunk (unset; reference default 24; only changes streaming iVector timing) */
  int32_t frame_subsampling_factor; /* --frame-subsampling-factor (unset; reference default 1.  f > 1: the decoder's frames are the output
                                     * rows t = 0, f, 2f, ...; frames_per_chunk is rounded up to a multiple of f: nnet-compile-looped.cc:81-94) */
  int32_t device_id;           /* HIP device ordinal */
  int32_t keep_intermediates;  /* 1: results keep features / iVectors / log-likelihoods for parity tests */
  int32_t max_tokens_per_frame;/* capacity of the per-frame token arrays on the device (0 = automatic) */
  int32_t emit_lattice;        /* 1: results keep the determinised lattice (rs_result_lattice); forces the lattice path */
  int32_t prune_output_pdfs;   /* 1 (default): evaluate the output layer only for the pdfs that occur on HCLG arcs (the search
                                * can read no others; transcripts and costs unchanged).  0 computes every pdf like the
                                * reference does.  Ignored with keep_intermediates and when the net ends in a log-softmax. */
  int32_t exact_token_order;   /* 1: the grammar-graph search creates tokens in the reference's order (the running `next_cutoff` of
                                * lattice-faster-decoder.cc:774-787 over its HashList order, hash-list-inl.h:125-165) -- costs equal the
                                * reference's on the frames where min-active / max-active binds, about 40 % more search time; graphs it
                                * does not apply to (more than 1000 states, chained epsilon arcs) are searched as with 0.  Default 0;
                                * RS_EXACT_ORDER=0|1 overrides. */
  int32_t command_line_fixed;  /* RS_FIXED_* bits: options whose only supported value was given ON THE COMMAND LINE (--online=false,
                                * --do-endpointing=false, --extra-left-context-initial=0, --prune-interval=25, --determinize-lattice=true).
                                * ParseOptions reads --config first and the command line overrides it (util/parse-options.cc:328-345), so
                                * an unsupported value of such an option in online.conf is then not an error.  rs_default_opts sets
                                * ONLINE | DO_ENDPOINTING: rhasspy's command line carries both (transcribe_wav.py:48-49). */
  int32_t stream_min_ticks;    /* rs_streams_advance coalescing: a call that brings fewer than this many new 1024-sample ticks (64 ms each) on EVERY
                                * listed stream does nothing and leaves the audio to the next call (the chunk / iVector schedule is a function
                                * of the samples accepted, not of the calls: results are the same for any value).  1: every call advances, the
                                * reference binary's per-tick cadence (online2-cli-nnet3-decode-faster.cc:143-161) -- lowest latency of
                                * rs_streams_finish, most launches; 0 = the library's default, 16 (about a second of audio per advance: the
                                * throughput setting).  RS_STREAM_MIN_TICKS=<n> overrides. */
  int32_t emit_alignment;      /* 1: results keep, per hypothesis, the transition-id of every decoder frame (rs_result_alignment, rs_result_phones):
                                * nbest-to-linear's second output.  0 (rs_default_opts): nothing is computed, kept or copied for it.  0 or 1 only --
                                * RS_OPT_UNSET is not a value (the reference has no such flag to take a value from): the model load refuses others. */
  int32_t reserved[1];
} rs_decode_opts;
#define RS_FIXED_ONLINE 1
#define RS_FIXED_DO_ENDPOINTING 2
#define RS_FIXED_EXTRA_LEFT_CONTEXT_INITIAL 4
#define RS_FIXED_PRUNE_INTERVAL 8
#define RS_FIXED_DETERMINIZE_LATTICE 16

/* Fills `opts` with the values the reference's Python passes / Kaldi defaults. */
int rs_default_opts(rs_decode_opts *opts);

/* Thread-local message of the last failing call on this thread ("" if none). */
const char *rs_last_error(void);

/* Replaces the per-process model loading of both binaries
 * (online2-wav-nnet3-latgen-faster.cc:150-190: OnlineNnet2FeaturePipelineInfo from --config=online.conf,
 * TransitionModel + AmNnetSimple from final.mdl, ReadFstKaldiGeneric(HCLG.fst)).  The base feature is online.conf's
 * --feature-type: mfcc (--mfcc-config) or fbank (--fbank-config: log-mel filterbank rows, up to 128 columns); only the selected
 * type's file counts and none means the type's defaults (online-nnet2-feature-pipeline.cc:28-56).  plp, pitch and VTLN warping are
 * refused with a message.  The network may start with TimeHeightConvolutionComponents (CNN-TDNN recipes) and a PermuteComponent;
 * refused with a message are a convolution whose required time offsets are a proper subset of its time offsets (zero padding in
 * time), one with more than 8 distinct time offsets or 128 output heights, one whose input rows of a frame exceed the kernel's 96 KiB
 * of LDS, and component types the HIP kernels do not implement.  The network may be recurrent where every cycle is what nnet3's
 * fast-lstmp-layer / fast-lstm-layer emit (TDNN-LSTM recipes): an affine W_all over Append(x, IfDefined(Offset(r_trunc, -d))), an
 * LstmNonlinearityComponent over Append(W_all, IfDefined(Offset(c_trunc, -d)) [, a 3-column DropoutMaskComponent node: all ones]),
 * optionally the projection W_rp over m, and one BackpropTruncationComponent (its <Scale> is honoured, here and anywhere else) whose
 * dim-ranges are the state; one delay d for both connections, 1 <= d <= 8, towards the past.  Limits: cell dim <= 2048, recurrent +
 * non-recurrent projection dim <= 4096, and 64 * (2 * recurrent input dim + cell dim [with a projection] + 12) bytes <= 144 KiB of
 * LDS.  A cycle without an LstmNonlinearityComponent may be the same cell spelled out, as lstmp-layer / lstmp-batchnorm-layer /
 * lstm-layer emit it: four affines of cell-dim rows over Append(x, IfDefined(Offset(r_t, -d))) with one x; the peepholes w_i.c and
 * w_f.c ((NaturalGradient)PerElementScaleComponent) over IfDefined(Offset(c_t, -d)), w_o.c over c_t; i_t, f_t, o_t SigmoidComponent
 * nodes over Sum(affine, peephole) [behind one shared DropoutComponent, a copy in test mode], g_t a TanhComponent over its affine,
 * h_t one over c_t; the ElementwiseProductComponents c1_t = Append(f_t, IfDefined(Offset(c_t, -d))), c2_t = Append(i_t, g_t), m_t =
 * Append(o_t, h_t); c_t a BackpropTruncationComponent (or ClipGradientComponent: scale 1) over Sum(c1_t, c2_t); r_t one over the
 * dim-range [0, R) of the affine W_rp.m over m_t, or over m_t; the two <Scale>s are honoured separately; the same delays and
 * limits; only rp_t and m_t may be read from outside the block.  Any other cycle -- an incomplete or differently wired cell of
 * that kind, a positive delay, two delays in one block, a block that reads another block's state at a future time --
 * is refused with the node and the reason.  A cycle around an LstmNonlinearityComponent may also be what lstmb-layer emits, the
 * cell behind a bottleneck: the LinearComponents W_all_a (bottleneck rows) over Append(x, IfDefined(Offset([Scale(s,)] m_trunc, -d)))
 * and W_all_b (4 x cell dim rows) over it, the ScaleAndOffsetComponent W_all_b_so of 4 x cell dim with vectors of that length
 * (applied as the component does: the scales through EnsureNonzero, multiply, then add), the nonlinearity over Append(W_all_b_so,
 * IfDefined(Offset(c_trunc, -d))) without a dropout mask, one BackpropTruncationComponent over its whole output whose dim-ranges
 * c_trunc / m_trunc are the state; Scale(s, ...) is accepted on this block's recurrent input only; only m, the nonlinearity's second
 * cell-dim columns, may be read from outside.  Limits: cell dim <= 2048, bottleneck dim <= 2048, 64 * (cell dim + bottleneck dim + 8)
 * bytes <= 144 KiB of LDS (dims rounded up to 16).  Outside a cycle a ScaleAndOffsetComponent is an ordinary scale / offset layer,
 * its block form (<Dim> a multiple of the vectors' length) included.  A
 * cycle may instead be what fast-opgru-layer / fast-norm-opgru-layer emit (TDNN-OPGRU recipes, the output-gate projected GRU): two
 * affines W_z, W_o of cell-dim rows over Append(x, IfDefined(Offset(s_t, -d))), each behind a SigmoidComponent [and one shared
 * DropoutComponent, a copy in test mode], an affine W_hpart over the same x, an OutputGruNonlinearityComponent over Append(z_t,
 * hpart_t, IfDefined(Offset(c_t, -d))) with c_t its second cell-dim columns, an ElementwiseProductComponent over Append(c_t, o_t),
 * the affine W_y, the dim-range [0, R) of W_y's node, optionally a NormalizeComponent (no add-log-stddev, no block-dim), and one
 * BackpropTruncationComponent whose node is s_t; a BatchNorm on W_y's node is an ordinary layer.  The same delays and the limits
 * cell dim <= 2048, R + P <= 4096, 64 * (2 * R + cell dim + 12) bytes <= 144 KiB of LDS (dims rounded up to 16).  Refused, in a
 * sentence of their own that names the node and the reason: anything else in a cycle that holds an OutputGruNonlinearityComponent.
 * Or a cycle may be what fast-pgru-layer / fast-norm-pgru-layer / fast-gru-layer emit (TDNN-PGRU recipes; the plain GRU): the
 * affines W_z (cell-dim rows) and W_r (R rows) over Append(x, IfDefined(Offset(s_t, -d))), each behind a SigmoidComponent [and a
 * DropoutComponent each, copies in test mode], W_hpart over the same x, a GruNonlinearityComponent (<CellDim>, <RecurrentDim> R,
 * <w_h> a cell x R matrix) over Append(z_t, r_t, hpart_t, IfDefined(Offset(c_t, -d)), IfDefined(Offset(s_t, -d))) with c_t its
 * second cell-dim columns, the affine W_y over c_t, the dim-range [0, R) of W_y's node, optionally a NormalizeComponent, and one
 * BackpropTruncationComponent whose node is s_t; fast-gru-layer: R = cell dim, a four-part input without c_t, no W_y, s_t the
 * truncation component over the nonlinearity's second cell-dim columns.  The same delays; cell dim <= 2048, R + P <= 4096,
 * 64 * (3 * R + cell dim + 16) bytes <= 144 KiB of LDS, without a projection 64 * (3 * cell dim + 12) bytes (dims rounded up to 16: a
 * cell dim of 752 at most).  Anything else in a cycle that holds a GruNonlinearityComponent is refused in that sentence, extended
 * by these three layers.  A cycle without any nonlinearity component but with a NoOpComponent node may be the GRU cell spelled
 * out, as the non-fast gru-layer / pgru-layer / norm-pgru-layer / opgru-layer / norm-opgru-layer emit it: y_t = NoOp(Sum(y1_t,
 * y2_t)) with the ElementwiseProductComponents y1_t = Append(h_t, Sum(Scale(-1.0, z_t), Const(1.0, cell-dim))) and y2_t =
 * Append(IfDefined(Offset(y_t, -d)), z_t) (gru-layer: Offset(s_t, -d)); z_t a SigmoidComponent [behind a DropoutComponent] over the
 * affine W_z.xs_z over Append(x, IfDefined(Offset(s_t, -d))); either h_t = Tanh(W_h.UW over Append(x, h1_t)), h1_t =
 * Append(r_t, IfDefined(Offset(s_t, -d))), r_t a gate of R rows (W_z.xs_r), or h_t = Tanh(Sum(W_h.UW over x, W_h.UW_elementwise over
 * IfDefined(Offset(y_t, -d)))), o_t a gate of cell-dim rows (W_z.xs_o), y_o_t = Append(o_t, y_t); s_t a BackpropTruncationComponent (or
 * ClipGradientComponent) over [a NormalizeComponent over] the dim-range [0, R) of the affine W_s.ys over y_t / y_o_t, in gru-layer
 * over y_t itself.  The same delays and limits as the fast blocks (a gru-layer: cell dim of 752 at most); only y_t, W_s.ys' node,
 * its dim-range and s_t may be read from outside the block; the cell is computed in that form's order, y = h (1 - z) + y[t-d] z
 * with every product and sum a rounding of its own.  Anything else in such a cycle is refused with the node and the reason in a
 * sentence that names the five layers; a Const() anywhere else is refused by name.  A cell of Sigmoid / Tanh / ElementwiseProduct
 * components without a NoOpComponent node is refused in the LSTM sentence: it is no complete lstmp-layer block.  The
 * rand() calls of a recurrent compilation are not replayed, so such a model loads only with --dither=0 in its mfcc.conf / fbank.conf
 * (rs_nnet3_setup below: certain = 0).  Parses on the host only;
 * the device copy is made on first use or by rs_model_to_device().  Immutable afterwards, shareable
 * between threads. */
int rs_model_load_files(const char *final_mdl, const char *hclg_fst, const char *online_conf,
                        const rs_decode_opts *opts, rs_model **out);
/* Same, using the directory layout the reference hard-codes (transcribe_wav.py:43-44,56-57):
 * <model_dir>/model/model/final.mdl, <model_dir>/model/online/conf/online.conf, <graph_dir>/HCLG.fst. */
int rs_model_load(const char *model_dir, const char *graph_dir, const rs_decode_opts *opts, rs_model **out);
int rs_model_to_device(rs_model *model);
void rs_model_free(rs_model *model);
/* Writes a one-line-per-item description of the parsed model (dims, layer plan, graph size) into buf;
 * returns the number of bytes needed (like snprintf).  The first line is the base feature's: `mfcc: win= shift= padded= mel_bins=
 * ceps= dither=`, or for a filterbank model `fbank: win= shift= padded= mel_bins= dim= use_energy= htk_compat= use_log= use_power=
 * dither=` (dim = mel_bins + use_energy, the width of a feature row).  After the `op:` lines comes one `conv:` line per convolution
 * (none for a model without one): name, filters in->out, heights in->out, height subsampling, offsets, distinct time offsets, k, the
 * kernel instantiation chosen at load, frames / pixel tiles / LDS bytes per workgroup, filter chunks, grid.  Then one `lstm:` line per
 * recurrent block: name, input dim, cell / recurrent / non-recurrent dims (0 / 0: no projection), delay, the truncation component's
 * scale, dropout_mask=0|1, the kernel instantiation, chains (rows) per workgroup, LDS bytes, the split of W_all's columns into
 * feed-forward + recurrent, cell and projection tiles, the grid rule.  Then one `lstmp:` line per block in the composed form
 * (lstmp-layer / lstm-layer), named after its node c_t: input dim, cell / recurrent / non-recurrent dims (0 / 0: lstm-layer), delay,
 * scale_c and scale_r (the two truncation components'), dropout=0|1 (the shared DropoutComponent), the kernel instantiation, chains
 * per workgroup, LDS bytes, the feed-forward (w_x) and recurrent (w_r) columns of each of the four affines, cell and projection
 * tiles, the grid rule; its `op: lstmp` line follows the `op: gemm <c_t>.x` of the four affines' stacked feed-forward columns
 * (4 x cell dim rows, gate order i, f, c, o).  Then one `lstmb:` line per block behind a bottleneck (lstmb-layer), named after its
 * nonlinearity's node: input dim, cell and bottleneck dims, delay, the truncation component's scale, self_scale (the Scale() on the
 * recurrent input), the kernel instantiation, chains per workgroup, LDS bytes, the split of W_all_a's columns (w_a), cell and
 * bottleneck tiles, the grid rule; its `op: lstmb` line follows the `op: gemm <W_all_a>.x` of W_all_a's feed-forward columns
 * (bottleneck rows, no bias).  Then one `gru:` line per GRU block: name, input dim, cell /
 * recurrent / non-recurrent dims, delay, the truncation component's scale, norm=0|1 (a NormalizeComponent in the recurrence),
 * dropout=0|1, the kernel instantiation, chains per workgroup, LDS bytes, the split of W_z's and W_o's columns, cell and output tiles,
 * the grid rule; its `op: gru` line follows the `op: gemm` of the stacked feed-forward columns (3 x cell dim rows).  Then one `pgru:` line per
 * block around a GruNonlinearityComponent: the same fields (rec=0 nonrec=0: fast-gru-layer), the split of W_z's and W_r's columns
 * (w_zr), cell, recurrent and output tiles; its `op: pgru` line follows the `op: gemm` of the stacked feed-forward columns (2 x cell
 * dim + R rows).  A GRU block in its composed form (opgru-layer / norm-opgru-layer; gru-layer / pgru-layer / norm-pgru-layer) prints as
 * its family's `gru:` / `pgru:` line, named after its node y_t, with kernel=gruc16x16x4<w8> / kernel=pgruc16x16x4<w8> and ` form=composed`
 * appended; a fast block's line is unchanged.  Two lines are state, not structure: `layer_gemm:` and
 *   arenas: device blocks=B bytes=N allocations=A; host blocks=B bytes=N allocations=A
 * summed over the model's decode contexts: the blocks and bytes their per-call arenas hold now, and the hipMalloc / hipHostMalloc
 * calls they have made since the model was loaded.  `allocations` stands still once every context has seen its largest call twice.
 * Once the model is on the device there is also
 *   search: states=S arcs_e=E arcs_x=X eps_depth=D max_out=Me,Mx reg=<nt,ke,kx> eps_rounds=R exact_ok=0|1 dense_ok=0|1
 *           dense_lattice=<nt,ka> crowded_at=N
 * (one line): what the search planner found on the graph -- states, emitting / epsilon arcs, the longest epsilon path (-1: cyclic; 0 also
 * beyond 5000 states, where nothing asks), the largest emitting / epsilon out-degree -- and decided at load: the register-resident
 * search's shape (reg=none: the graph fits none), its closure rounds (-1: until nothing changes), whether exact_token_order applies,
 * whether the LDS-resident dense search does, the lattice kernel of an n-best call (none: the graph is beyond its 2048 states / 8192
 * arcs), and the smallest batch that gets the crowded shape (half the waves, twice the arcs per thread: 4 n_utts >= 3 CUs).
 * A model opened with keep_intermediates = 1 also prints, for every distinct layer GEMM its most recent decode call or stream advance
 * launched (in launch order; the iVector branch's two splice + LDA launches included)
 *   gemm_launch: <op name> rows=R n=N ksteps=K <kernel> blocks=B threads=T nbig=F nfirst=S res=0|1 img=0|1
 * the op as on its `op:` line (the name may hold blanks), the rows and columns of the product, the 16-wide k-steps of the split-fp16
 * k loop, the kernel instantiation by its template arguments -- Exact<MT,WM,WN,vec,dma>, B3<MR,MIXED,WM>, B3I<MR,MIXED,KPS> or
 * B3J<WM,MIXED,STRIP,SDIV,MRT,WN> -- the grid, the full-height row tiles, the small tiles launched in front of them, whether a
 * residual pass follows the kernel and whether the launch writes the operand image.  With keep_intermediates = 0 nothing is recorded
 * and no such line is printed. */
int rs_model_describe(const rs_model *model, char *buf, size_t len);
/* The check the reference makes when a waveform arrives (OnlineGenericBaseFeature::MaybeCreateResampler, feat/online-feature.cc:
 * 86-101; online2-wav-nnet3-latgen-faster.cc:233 hands it WaveData::SampFreq()): RS_OK when `sample_rate` is the model's
 * --sample-frequency, else an error whose text is Kaldi's "Sampling frequency mismatch, expected 16000, got 8000 ...".  The PCM entry
 * points below take samples, not files: a caller that read a wav header calls this first (rhasspy_speech_amd.transcribe_wav and the
 * online2-wav-nnet3-latgen-faster shim do).  --allow-downsample / --allow-upsample in mfcc.conf / fbank.conf (the reference then resamples) are
 * refused with a message: the library does not resample. */
int rs_model_check_sample_rate(const rs_model *model, float sample_rate);
/* *out = the model's --sample-frequency (mfcc.conf / fbank.conf; 16000 without the line).  Every PCM entry point -- rs_decode_batch*,
 * rs_stream_accept* -- takes samples AT THAT RATE and never sees a rate: 8 kHz telephone models (a 200-sample window, a 256-point
 * transform) take 8 kHz audio, and so on.  Windows that pad to 256, 512, 1024 or 2048 points load; a caller whose audio carries a
 * rate (a wav header, the stream binary's --samp-freq) compares it with rs_model_check_sample_rate before handing samples over. */
int rs_model_sample_rate(const rs_model *model, float *out);

/* Offline batch decode = N invocations of the reference's 3-process pipeline with --online=false
 * (online2-wav-nnet3-latgen-faster.cc:196-300 + lattice-to-nbest.cc:80-110 + nbest-to-linear.cc:67-87).
 * pcm[i] points to n_samples[i] mono int16 samples at the model's rate (rs_model_sample_rate; WaveData::Read hands Kaldi the same
 * values as floats, unscaled).  nbest = lattice-to-nbest --n; lattice_acoustic_scale = its --acoustic-scale. */
int rs_decode_batch(rs_model *model, const int16_t *const *pcm, const int32_t *n_samples, int32_t n_utts,
                    int32_t nbest, float lattice_acoustic_scale, rs_result **out);
/* Same with the samples already resident in device memory (HBM): d_pcm is one device buffer holding all
 * utterances back to back, sample_offsets[i] (host array, n_utts+1 entries) delimits utterance i.
 * stream = hipStream_t to run on (NULL = the model's own stream).  This is what bench.py times. */
int rs_decode_batch_device(rs_model *model, const int16_t *d_pcm, const int64_t *sample_offsets,
                           int32_t n_utts, int32_t nbest, float lattice_acoustic_scale, void *stream,
                           rs_result **out);

/* Streaming decode = online2-cli-nnet3-decode-faster (stdin s16le at the model's rate until EOF, :143-161; its --samp-freq is
 * the caller's to check, rs_model_check_sample_rate) followed by
 * lattice-to-nbest | nbest-to-linear (transcribe_stream.py:85-99).  Audio may arrive in arbitrary chunk
 * sizes; the library re-chunks to the binary's fixed 1024-sample ticks (:37) so results do not depend on
 * the caller's chunking, exactly like the reference. */
int rs_stream_open(rs_model *model, rs_stream **out);
int rs_stream_accept(rs_stream *stream, const int16_t *pcm, int32_t n_samples);
int rs_stream_finish(rs_stream *stream, int32_t nbest, float lattice_acoustic_scale, rs_result **out);
void rs_stream_free(rs_stream *stream);
/* Many concurrent streams (BASELINE.json config 5).  The reference's streaming result is a deterministic function
 * of the sample sequence: which frames each nnet chunk's iVector has seen follows from the 1024-sample tick
 * schedule alone (decodable-online-looped.cc:56-84,186-194), not from wall-clock time.  The library therefore
 * reproduces it exactly from the samples accepted so far: rs_streams_advance does, batched over the listed streams, all the
 * device work those samples make possible (MFCC of the completed frames, the iVector estimates and nnet chunks of the ticks
 * reached, the search over the new rows -- what online2-cli-nnet3-decode-faster.cc:143-161 does per tick), so that
 * rs_streams_finish (stdin EOF for all listed streams) only has the tail left; result utterance i belongs to streams[i].
 * A call that finds less than 16 ticks (1 s) of new audio on every listed stream leaves them to the next call: an advance is
 * chains of small dependent launches whose length hardly depends on the rows, and nothing but the end of a stream reads its
 * results -- same rows, same results, a third fewer milliseconds per hour of audio (RS_STREAM_MIN_TICKS=1: every call works).
 * An advance that fails leaves the streams it listed unusable (every later call on them except rs_stream_free is refused). */
int rs_streams_accept(rs_stream *const *streams, const int16_t *const *pcm, const int32_t *n_samples, int32_t n_streams);
    /* rs_stream_accept for many streams in one call: pcm[i] / n_samples[i] go to streams[i] (a host that serves hundreds of streams
     * hands over a round of audio per call; the samples are copied, like stdin is read, online2-cli-nnet3-decode-faster.cc:143-148) */
int rs_streams_advance(rs_stream *const *streams, int32_t n_streams);
int rs_streams_finish(rs_stream *const *streams, int32_t n_streams, int32_t nbest, float lattice_acoustic_scale,
                      rs_result **out);
/* Partial results = SingleUtteranceNnet3Decoder::GetBestPath(end_of_utterance = false) (online-nnet3-decoding.cc:82-85), what
 * online2-tcp-nnet3-decode-faster prints as its temporary transcript.  rs_streams_partial does, batched over the listed streams, the
 * device work rs_streams_advance would do -- for every completed tick, without the 16-tick coalescing -- then returns, per stream,
 * the best path over the decoder frames searched so far with NO final costs: an ordinary rs_result with one hypothesis per stream
 * (utterance i = streams[i]): words = the non-zero output labels along the path, graph / acoustic cost with the per-frame cost
 * offsets removed (TraceBackBestPath), rs_result_num_frames = the decoder frames searched so far (NumFramesDecoded()).  A stream
 * with no decoded frame yet gets 0 words, cost 0 and 0 frames, status RS_OK (the reference asserts there).  The streams stay open,
 * and a later rs_streams_finish gives bit for bit what it gives without the partial calls.  A finished, freed or failed stream is
 * refused like by the other stream calls; so are streams opened with RS_STREAM_BATCH=1.
 * Ties between equal frontier costs go to the lowest state index (the reference keeps the first token of its list).
 * rs_result_counters out[0] of a partial result = back-pointer rows the traceback read; out[1..6] = 0.
 * Cost: on grammar graphs the register-resident search holds (<= 5000 states), the traceback reads the rows between the frontier and
 * the point where the best path joins the previous call's best path (cached per stream), not the whole stream while the best
 * hypothesis holds (RS_PARTIAL_FULL_WALK=1: always the whole stream, same results).  For streams whose search is deferred to
 * finish (larger graphs, RS_DECODER=dense|sparse|hash) a partial runs that search over all frames so far: O(frames) per call. */
int rs_streams_partial(rs_stream *const *streams, int32_t n_streams, rs_result **out);
int rs_stream_partial(rs_stream *stream, rs_result **out);

/* Endpointing = online2/online-endpoint.{h,cc}: has the speaker stopped?  Five rules over the trailing silence of the best path so
 * far, the final relative cost and the utterance length (OnlineEndpointConfig, online-endpoint.h:128-186).  The reference's stream
 * binary registers the config on the parser that reads online.conf (online2-cli-nnet3-decode-faster.cc:76), which is why
 * --endpoint.* lines may stand there; online2-wav-nnet3-latgen-faster asks after every chunk and breaks at a detection (:270-274).
 * --do-endpointing=true / --online=true in online.conf are still refused at load: the entry points below are how a caller asks. */
typedef struct rs_endpoint_rule {          /* OnlineEndpointRule, online-endpoint.h:52-71 */
  int32_t must_contain_nonsilence;         /* --endpoint.ruleN.must-contain-nonsilence */
  float min_trailing_silence;              /* --endpoint.ruleN.min-trailing-silence, seconds */
  float max_relative_cost;                 /* --endpoint.ruleN.max-relative-cost */
  float min_utterance_length;              /* --endpoint.ruleN.min-utterance-length, seconds */
} rs_endpoint_rule;
#define RS_ENDPOINT_SILENCE_CHARS 4096
typedef struct rs_endpoint_opts {
  rs_endpoint_rule rule[5];                /* rule1 .. rule5 */
  char silence_phones[RS_ENDPOINT_SILENCE_CHARS]; /* --endpoint.silence-phones: colon-separated phone ids, NUL-terminated ("" = none given) */
  int32_t reserved[4];
} rs_endpoint_opts;
/* The defaults of online-endpoint.h:152-157: rule1 {false, 5.0, inf, 0}, rule2 {true, 0.5, 2.0, 0}, rule3 {true, 1.0, 8.0, 0},
 * rule4 {true, 2.0, inf, 0}, rule5 {false, 0, inf, 20.0}; no silence phones. */
int rs_default_endpoint_opts(rs_endpoint_opts *opts);
/* The defaults overridden by the --endpoint.silence-phones / --endpoint.rule{1..5}.{must-contain-nonsilence, min-trailing-silence,
 * max-relative-cost, min-utterance-length} lines of the model's online.conf (booleans and numbers parsed like the file's other
 * options; a repeated option: the last one wins).  A value that does not parse does not fail the model load: it fails this call,
 * and every endpoint call that uses the model's options, with the parser's message. */
int rs_model_endpoint_opts(const rs_model *model, rs_endpoint_opts *opts);
/* EndpointDetected(config, num_frames_decoded, trailing_silence_frames, frame_shift_in_seconds, final_relative_cost)
 * (online-endpoint.cc:46-72) on the host, no device involved: 0, or the number 1..5 of the first rule that fires.  In float like
 * the reference (BaseFloat): utterance_length = frames * shift, trailing_silence = silence frames * shift, contains_nonsilence =
 * utterance_length > trailing_silence (RuleActivated, :26-44).  The silence list is not looked at.  -1 for a null `opts`. */
int rs_endpoint_rule_fired(const rs_endpoint_opts *opts, int32_t num_frames_decoded, int32_t trailing_silence_frames,
                           float frame_shift_seconds, float final_relative_cost);
typedef struct rs_endpoint_status {
  int32_t detected;                /* 0, or the first rule that fired (1..5) */
  int32_t num_frames_decoded;      /* NumFramesDecoded() */
  int32_t trailing_silence_frames; /* TrailingSilenceLength() */
  float   final_relative_cost;     /* FinalRelativeCost(); +inf if no frontier token is final */
  float   frame_shift_seconds;     /* feature frame shift x frame-subsampling-factor */
  int32_t rows_read;               /* back-pointer rows (frames) the trailing-silence walk read: trailing_silence_frames + 1 on grammar
                                    * graphs (0 before the first decoded frame), the counterpart of a partial's rs_result_counters out[0] */
} rs_endpoint_status;
/* EndpointDetected(config, tmodel, frame_shift, decoder) (online-endpoint.cc:109-126; SingleUtteranceNnet3Decoder::EndpointDetected,
 * online-nnet3-decoding.cc:88-95) for the listed streams of one model.  The call first does what rs_streams_partial does first: the
 * device work of every completed 1024-sample tick, no coalescing, batched -- so the answer is a function of the samples accepted,
 * not of how the caller called.  Then per stream (out[i] = streams[i]):
 *   num_frames_decoded      = decoder frames searched so far.  0: detected = 0, no silence, cost +inf, RS_OK (:115);
 *   final_relative_cost     = min over the frontier's tokens of cost + Final(state), minus the min of cost; +inf when no frontier state
 *                             is final or no token survives (lattice-faster-decoder.cc:536-569);
 *   trailing_silence_frames = from the best frontier token WITHOUT final costs (rs_streams_partial's token, ties to the lowest state)
 *                             backwards: input-epsilon arcs are skipped, an emitting arc whose transition-id belongs to a phone of the
 *                             silence list counts one, the first other emitting arc ends the walk (online-endpoint.cc:89-106);
 *   frame_shift_seconds     = mfcc.conf's (fbank.conf's) --frame-shift in seconds x --frame-subsampling-factor (online-nnet3-decoding.cc:88-95);
 *   detected                = rs_endpoint_rule_fired of these.
 * opts = NULL: the model's (rs_model_endpoint_opts).  An empty silence list fails with RS_ERR_ARG "Endpointing requires nonempty
 * --endpoint.silence-phones option", one that does not parse or holds a phone twice with "Bad --silence-phones option in endpointing
 * config: ..." (online-endpoint.cc:79-86).  Nothing a partial, an advance or a finish reads is written: what they return afterwards
 * is bit for bit what they return without the endpoint calls.  Finished, freed, failed and RS_STREAM_BATCH=1 streams are refused
 * as by rs_streams_partial.  A stream whose search has failed (a partial reports RS_ERR_DECODE for that utterance: no surviving
 * tokens, token capacity exceeded, epsilon cycle) has no answer: the call returns RS_ERR_DECODE with "rs_streams_endpoint: stream i:
 * <the partial's message>", every record's `detected` is 0, and the streams stay usable as after such a partial.  A frontier that
 * is healthy but holds no final state gives cost +inf and RS_OK.
 * Cost: on grammar graphs the register-resident search holds, one workgroup per stream reduces the parked frontier twice and walks
 * the back-pointer rows of the trailing silence plus one.  The walk is serial -- one lane, one dependent load chain per row -- and
 * nothing is cached between calls, so a query costs time linear in the trailing silence at that moment: short while somebody
 * speaks, growing by one row per frame for as long as a pause lasts (500 rows at 10 ms frames when rule1's default 5 s fire), and
 * the whole stream if the silence list covers every phone of the best path.  The "is silence" table it reads is a device
 * bitmap over the graph's arcs (the device arcs carry pdf ids, so the arc's transition-id -> phone lookup is done when the bitmap is
 * built), made once per model and silence list and kept while the list stays the same.  For streams whose search is deferred to
 * finish (larger graphs, RS_DECODER=dense|sparse|hash) the call runs the token-list search over all frames so far and reads that
 * search's last frame and back pointers: O(frames) per call, like their partials. */
int rs_streams_endpoint(rs_stream *const *streams, int32_t n_streams, const rs_endpoint_opts *opts, rs_endpoint_status *out);
int rs_stream_endpoint(rs_stream *stream, const rs_endpoint_opts *opts, rs_endpoint_status *out);
/* What the reference does once an endpoint is detected: it stops reading audio and calls FinalizeDecoding() + GetLattice(true) on the
 * frames decoded so far WITHOUT InputFinished() (online2-wav-nnet3-latgen-faster.cc:270-278) -- no flush of the feature tail, which
 * rs_streams_finish always does.  rs_streams_finalize does the catch-up of rs_streams_endpoint, then everything rs_streams_finish
 * does after its flush (final costs, lattice, determinisation, n-best, emit_lattice) over exactly the decoder frames searched;
 * rs_result_num_frames reports them.  Samples beyond the last complete tick are ignored as if never accepted.  The streams are
 * finished afterwards.  A stream without a decoded frame fails like the decode of an empty utterance. */
int rs_streams_finalize(rs_stream *const *streams, int32_t n_streams, int32_t nbest, float lattice_acoustic_scale,
                        rs_result **out);
int rs_stream_finalize(rs_stream *stream, int32_t nbest, float lattice_acoustic_scale, rs_result **out);

/* Speaker adaptation = what online2-wav-nnet3-latgen-faster carries from one utterance of a speaker to the next
 * (OnlineIvectorExtractorAdaptationState + OnlineCmvnState, :203-205 construct them per speaker, :220-221 set them on the feature
 * pipeline before an utterance, :287-288 read them back after it).  A state is a small host object of doubles:
 *   RS_ADAPT_IVECTOR_LINEAR     the iVector estimator's linear term, ivector_dim;
 *   RS_ADAPT_IVECTOR_QUADRATIC  its quadratic term, the packed lower triangle row by row, ivector_dim (ivector_dim + 1) / 2;
 *   RS_ADAPT_IVECTOR_COUNT      its num_frames, 1;
 *   RS_ADAPT_CMVN_IVECTOR       speaker CMVN statistics of the iVector branch, 2 x (feat_dim + 1): row 0 = sum x | count, row 1 = sum x^2 | 0;
 *   RS_ADAPT_CMVN_NNET          the same for the nnet-input CMVN (--cmvn-config in online.conf), where the model has one.
 * Blocks the model has no use for (no extractor: the first four; no nnet-input CMVN: the last) are empty.
 *
 * rs_adaptation_new: the fresh-speaker state (the estimator as constructed, no speaker statistics).  No device involved.
 * rs_streams_adaptation: one new state per listed stream (out[i] = streams[i]; free each with rs_adaptation_free), in one batched
 *   device pass and one copy to the host.  The streams have ENDED -- rs_streams_finish or rs_streams_finalize returned RS_OK for
 *   them -- and are not freed yet.  What it computes (OnlineIvectorFeature::GetAdaptationState, online-ivector-feature.cc:386-396):
 *     - the CMVN statistics the stream was opened with plus (1, x, x^2) per raw MFCC frame in frame order, in double
 *       (OnlineCmvn::GetState, online-feature.cc:467-487): every frame after a finish; after a finalize the frames of the complete
 *       ticks (samples beyond the last complete tick are ignored there too);
 *     - the estimator's statistics as they stand;
 *     - LimitFrames(--max-remembered-frames, --posterior-scale) (online-ivector-feature.cc:109-127): the iVector-branch CMVN block
 *       is scaled by max_remembered_frames / count where the count is above it, the estimator's statistics by max_remembered_frames x
 *       posterior_scale / num_frames where above that, with the prior term re-added on element 0 and the diagonal
 *       (OnlineIvectorEstimationStats::Scale, ivector-extractor.cc:671-693: --max-count = 0 and > 0).  The nnet-input block is never
 *       limited.  The scalings are done in double (the reference rounds the CMVN factor to float: 6e-8 relative).
 *   An ended stream keeps its place in the model's stream pool until rs_stream_free.  Should the pool run out of slots or rows
 *   meanwhile, the oldest ended streams give theirs up, and asking for their state then fails with RS_ERR_ARG -- so take the state
 *   before opening many more streams, and free ended streams as before.
 * rs_stream_open_adapted: rs_stream_open with the state set before the first frame (SetAdaptationState, :445-453: the estimator's
 *   statistics are replaced, its solution starts from [prior_offset, 0, ...] as always; SetCmvnState).  From then on the stream's
 *   CMVN adds min(cmn_window - n, speaker_frames, speaker count) / speaker count x the speaker statistics before the global part
 *   (SmoothOnlineCmvnStats, online-feature.cc:372-419).  state == NULL is rs_stream_open; a fresh state gives the same stream bit
 *   for bit.  The state is copied: it may be freed or reused for other streams at once.  Dither noise is the fresh-process
 *   sequence for every stream, adapted or not.
 * rs_adaptation_export: block `what` into buf (cap doubles); *n = its length, also when buf is NULL or cap too small (RS_ERR_ARG then).
 * rs_adaptation_import: a state from such arrays (a NULL pointer with length 0 = an empty block), to carry a speaker across
 *   processes.  Lengths must be the model's, counts not negative, every value finite.
 * Refused with RS_ERR_ARG and a message, the streams staying as usable as they were: a stream that has not ended, a failed stream,
 * an RS_STREAM_BATCH=1 stream (and opening one with a state other than NULL), a state whose dimensions are not the model's. */
typedef struct rs_adaptation rs_adaptation;
enum { RS_ADAPT_IVECTOR_LINEAR = 0, RS_ADAPT_IVECTOR_QUADRATIC = 1, RS_ADAPT_IVECTOR_COUNT = 2, RS_ADAPT_CMVN_IVECTOR = 3, RS_ADAPT_CMVN_NNET = 4 };
int rs_adaptation_new(const rs_model *model, rs_adaptation **out);
int rs_streams_adaptation(rs_stream *const *streams, int32_t n_streams, rs_adaptation **out);
int rs_stream_adaptation(rs_stream *stream, rs_adaptation **out);
int rs_stream_open_adapted(rs_model *model, const rs_adaptation *state, rs_stream **out);
int rs_adaptation_export(const rs_adaptation *a, int32_t what, double *buf, int64_t cap, int64_t *n);
int rs_adaptation_import(const rs_model *model, const double *ivector_linear, int64_t n_linear, const double *ivector_quadratic, int64_t n_quadratic,
                         double ivector_count, const double *cmvn_ivector, int64_t n_cmvn_ivector, const double *cmvn_nnet, int64_t n_cmvn_nnet,
                         rs_adaptation **out);
void rs_adaptation_free(rs_adaptation *a);

/* Result access.  Hypotheses of utterance `utt` are ordered best first, like the keys utt-1..utt-n that
 * lattice-to-nbest writes (lattice-to-nbest.cc:100-106). */
int32_t rs_result_num_utts(const rs_result *r);
int32_t rs_result_num_hyps(const rs_result *r, int32_t utt);
int32_t rs_result_num_frames(const rs_result *r, int32_t utt);
/* Word ids (HCLG olabels, epsilons removed) of hypothesis k; *ids stays valid until rs_result_free. */
int rs_result_words(const rs_result *r, int32_t utt, int32_t k, const int32_t **ids, int32_t *n);
/* The utterance's lattice as one binary CompactLattice table entry ("<key> " + VectorFst<CompactLatticeArc> with no "\0B" marker,
 * lat/kaldi-lattice.cc:62-70,:478-500, fstext/lattice-weight.h:141-145,:471-475,:532-540): what online2-wav-nnet3-latgen-faster
 * writes to its `ark:` wspecifier (online2-wav-nnet3-latgen-faster.cc:286-300), i.e. the bytes the reference pipes into
 * lattice-to-nbest.  Needs rs_decode_opts.emit_lattice = 1.  The lattice is determinised on words within lattice_beam and
 * is equivalent to the reference's (same word sequences, costs and best alignments), not byte-identical: state numbering
 * is this library's.  Returns the entry's size in bytes (copies min(size, cap) bytes to buf), or a negative error. */
int64_t rs_result_lattice(const rs_result *res, int32_t utt, const char *key, char *buf, int64_t cap);

/* (graph cost, acoustic cost) of hypothesis k = the 4th/5th outputs of nbest-to-linear. */
int rs_result_costs(const rs_result *r, int32_t utt, int32_t k, float *graph_cost, float *acoustic_cost);
/* Renders exactly the bytes `nbest-to-linear ark:- ark:/dev/null ark,t:-` prints for this utterance:
 * "utt-<k> <id> <id> ... \n" per hypothesis (key prefix `key`, "utt" in the reference).  Returns the number
 * of bytes needed, like snprintf. */
int rs_result_text(const rs_result *r, int32_t utt, const char *key, char *buf, size_t len);
/* Alignments = the second output of nbest-to-linear (nbest-to-linear.cc:67-87: GetLinearSymbolSequence's input labels), which the
 * reference sends to ark:/dev/null.  Needs rs_decode_opts.emit_alignment = 1; without it all three calls return RS_ERR_ARG with a
 * message that names the option.  Results of rs_streams_partial carry none (RS_ERR_ARG: the partial traceback joins a cached path
 * instead of walking every frame), nor do the records of rs_decode_batch_sharded (they are not rs_result objects).
 * rs_result_alignment: the transition-ids of hypothesis k, one per DECODER frame (*n == rs_result_num_frames; with
 *   --frame-subsampling-factor=f one per f feature frames) -- what the reference writes for key utt-<k+1>.  *tids stays valid until
 *   rs_result_free.  A 1-best call without a lattice (nbest = 1, lattice scale 1, no emit_lattice) takes them from the search's own
 *   traceback on the device; every other call from the lattice: the best alignment of the word sequence, ties of bit-identical
 *   (total, graph) cost going to the shorter, then lexicographically smaller string (CompactLatticeWeight's order).
 * rs_result_alignment_text: exactly the bytes `nbest-to-linear ark:- ark,t:- ark:/dev/null` prints ("<key>-<k> tid tid ... \n" per
 *   hypothesis); returns the number of bytes needed, like rs_result_text.
 * rs_result_phones: the alignment split into phones as SplitToPhones does (hmm/hmm-utils.cc:659-732; what `ali-to-phones
 *   --write-lengths` prints): segment i is phone[i] over decoder frames [start_frame[i], start_frame[i] + num_frames[i]).  Host work
 *   on the transition model the result's model was loaded with, following the reordered self-loop convention of graphs built with
 *   --reorder=true (a phone's final transition-id may be followed by self-loops of the same transition-state).  An alignment that
 *   does not split cleanly -- an rs_streams_finalize may end inside a phone -- fails with RS_ERR_DECODE and the reference's warning
 *   "Could not split word into phones correctly (forced-out?)" (word-align-lattice-lexicon.cc:752), not with a guess. */
int rs_result_alignment(const rs_result *r, int32_t utt, int32_t k, const int32_t **tids, int32_t *n);
int rs_result_alignment_text(const rs_result *r, int32_t utt, const char *key, char *buf, size_t len);
int rs_result_phones(const rs_result *r, int32_t utt, int32_t k, const int32_t **phone, const int32_t **start_frame, const int32_t **num_frames,
                     int32_t *n);

/* Fixed-size result records of the best hypothesis of every utterance, for the multi-GPU gather (one RCCL
 * all_gather of these records is the path's only exchange step): out[u * (max_words + 4)] =
 * {status (0 ok), n_words, word ids (max_words slots, truncated), graph cost bits, acoustic cost bits}. */
int rs_result_pack(const rs_result *r, int32_t max_words, int32_t *out);
/* Multi-GPU entry point (BASELINE.json configs[3]: a batch whose utterances name different
 * models, sharded over the GPUs of one node).  The reference runs one process per utterance with no shared state
 * (rhasspy_speech/tools.py:117-147), so the partition is free: utterance i belongs to rank i % world.  Every rank calls this
 * with the same utt_model[] / n_utts (one process per GPU; models[m] resident on this rank's device); pcm[i] / n_samples[i]
 * need only be valid for the rank's own utterances.  The rank decodes its utterances -- one device batch per model, the
 * models' batches concurrently -- and ONE ncclAllGather over `rccl_comm` (an ncclComm_t whose rank / size are `rank` /
 * `world`; RCCL over xGMI) fills `records` (n_utts x RS_SHARD_RECORD_INTS int32) for EVERY utterance on every rank:
 *   [0] utterance index, [1] status (RS_OK, a negative RS_ERR_*, or RS_SHARD_ABSENT), [2] number of words of the 1-best (if it
 *   exceeds RS_SHARD_MAX_WORDS the ids were cut), [3 .. 3+RS_SHARD_MAX_WORDS) word ids, then graph / acoustic cost (float bits).
 * Failures travel in the status field and the collective always runs, so a failing rank cannot leave the others waiting;
 * the return value is this rank's first failure (after the gather).  With rccl_comm = NULL no collective is
 * issued and only the rank's own records are filled (the others read RS_SHARD_ABSENT): for callers that gather themselves. */
#define RS_SHARD_MAX_WORDS 63
#define RS_SHARD_RECORD_INTS (3 + RS_SHARD_MAX_WORDS + 2)   /* 68 int32 = 272 bytes */
#define RS_SHARD_ABSENT 1
int rs_decode_batch_sharded(rs_model *const *models, int32_t n_models, const int32_t *utt_model, const int16_t *const *pcm,
                            const int32_t *n_samples, int32_t n_utts, int32_t rank, int32_t world, void *rccl_comm,
                            int32_t *records);
/* The exchange step of rs_decode_batch_sharded on its own: `records` holds this rank's records at their utterance indices (what
 * rs_decode_batch_sharded leaves when called with rccl_comm = NULL); ONE ncclAllGather over `rccl_comm` later it holds every
 * rank's.  For hosts that keep several decode calls in flight: the collectives of one communicator must be issued in the same
 * order on every rank, so such a host decodes from its worker threads and gathers from one thread in step order.  The
 * reference has no counterpart (one process per utterance, tools.py:117-147); `device_id` = the rank's GPU. */
int rs_shard_gather(int32_t device_id, int32_t n_utts, int32_t rank, int32_t world, void *rccl_comm, int32_t *records);
/* Host-side placement for one-process-per-GPU hosts (no counterpart in the reference, which never shares a box between GPUs):
 * restricts the CALLING thread -- and every thread it creates afterwards, the library's own helper threads included -- to the
 * CPUs local to GPU `device_id` (`/sys/bus/pci/devices/<bus id>/local_cpulist`: the cores of its NUMA node), so that a rank's
 * staging copies (24.6 MB of PCM per 2.3 ms step on the headline workload) read and write node-local memory instead of crossing
 * the socket interconnect at eight ranks.  Returns the number of CPUs in the mask (0: the system names none -- nothing changed),
 * or a negative RS_ERR_*.  RS_BIND_CPULIST=<list> (e.g. "0-15,64-79") overrides the list and needs no device. */
int rs_bind_host_thread(int32_t device_id);

/* Parity taps (only with opts.keep_intermediates): kind 0 = nnet input features (T x C), 1 = iVector
 * (n x D_iv: one row offline, one row per nnet chunk for streams), 2 = log-likelihoods (T x P); 3 + k = the output of the
 * model's k-th convolution (T x heights * filters, ReLU and BatchNorm applied; batch calls only); 64 + k = the output rows of the
 * model's k-th recurrent block of any kind, in network order, what the layers above it read (an LSTM block of either form: T x (recurrent +
 * non-recurrent) dim: rp / rp_t, before any BatchNorm; or T x cell dim: m / m_t, without a projection; an lstmb-layer block: T x cell
 * dim: m, before m_batchnorm; an OPGRU or PGRU block of either form: T x (recurrent +
 * non-recurrent) dim: W_y's / W_s.ys' rows, before any BatchNorm; a fast-gru-layer or gru-layer block: T x cell dim: c / y_t; batch calls only; under --frame-subsampling-factor only the rows the block was walked on
 * hold anything); 128 + k = the output rows of the model's k-th RestrictedAttentionComponent, in network order (T x heads *
 * (value-dim [+ num-left-inputs + 1 + num-right-inputs with output-context]): per head the weighted values, then the softmax
 * weights; before the ReLU / BatchNorm / Normalize nodes behind it; batch calls only; under --frame-subsampling-factor only the rows
 * the op was evaluated on hold anything). */
int rs_result_matrix(const rs_result *r, int32_t utt, int32_t kind, const float **data, int32_t *rows, int32_t *cols);
/* Decoder work counters of one utterance, for the algorithmic-bytes figure of SURVEY.md section 8(d):
 * out[0] = tokens expanded, [1] = arcs examined, [2] = token insertions (FindOrAddToken calls),
 * [3] = tokens alive summed over frames, [4] = lattice arcs after pruning, [5] = frames where
 * max_active bound, [6] = frames where min_active bound, [7] = token-capacity overflows. */
int rs_result_counters(const rs_result *r, int32_t utt, int64_t out[8]);
/* Wall-clock milliseconds of the stages of the call that produced r: out[0] = H2D, [1] = MFCC,
 * [2] = iVector, [3] = nnet, [4] = decode, [5] = lattice+n-best (host), [6] = total.  For a result of rs_streams_finish the
 * stages are summed over the finishing call and the rs_streams_advance calls that preceded it on the model, and out[7] is the
 * wall time of the finishing call alone. */
int rs_result_timings(const rs_result *r, float out[8]);
void rs_result_free(rs_result *r);

/* ---- fuzzy matching of an n-best list against <lang_dir>/G.fuzzy.fst (host side, no GPU involved).
 * Replaces rhasspy_speech/transcribe_util.py:11-88 (`get_fuzzy_text`: the n-best text piped through fstcompile |
 * fstcompose - G.fuzzy.fst | fstshortestpath | fstrmepsilon | fsttopsort | fstproject | fstprint, then the printed arcs
 * summed in Python).  rs_fuzzy_open parses the FST once (the reference re-reads it per utterance). */
typedef struct rs_fuzzy rs_fuzzy;
int rs_fuzzy_open(const char *fuzzy_fst_path, rs_fuzzy **out);
/* nbest_text = the bytes rs_result_text() renders (`utt-k id id ...` lines).  On a match *n_out = number of output labels
 * (<= cap written to olabels, word ids of <lang_dir>/words.txt incl. `__output:` meta words, epsilons removed) and *cost =
 * the value the reference compares with max_fuzzy_cost; *n_out = -1 when the reference would return None. */
int rs_fuzzy_match(const rs_fuzzy *f, const char *nbest_text, int32_t *olabels, int32_t cap, int32_t *n_out, double *cost);
/* The same match taken straight from a decode result (utterance `utt` of r): what transcribe_wav.py:87-93 /
 * transcribe_stream.py:117-123 do with the pipeline's stdout, without rendering and re-parsing the n-best text. */
int rs_result_fuzzy(const rs_result *r, int32_t utt, const rs_fuzzy *f, int32_t *olabels, int32_t cap, int32_t *n_out, double *cost);
void rs_fuzzy_free(rs_fuzzy *f);

/* ---- decoding-graph construction (host side).
 * Replaces `bash utils/mkgraph.sh --self-loop-scale 1.0 <lang_dir> <model_dir>/model <graph_dir>` (rhasspy_speech/kaldi.py:409-425;
 * kaldi/egs/wsj/s5/utils/mkgraph.sh:72-170), i.e. the process chain
 *   fsttablecompose L_disambig.fst G.fst | fstdeterminizestar --use-log=true | fstminimizeencoded | fstpushspecial   (LG)
 *   fstcomposecontext --context-size=N --central-position=P ... | fstarcsort --sort_type=ilabel                      (CLG, N / P from `tree`)
 *   make-h-transducer --transition-scale=<transition_scale> ilabels tree final.mdl                                   (Ha)
 *   fsttablecompose Ha CLG | fstdeterminizestar --use-log=true | fstrmsymbols | fstrmepslocal | fstminimizeencoded   (HCLGa)
 *   add-self-loops --self-loop-scale=<self_loop_scale> --reorder=true final.mdl | fstconvert --fst_type=const        (HCLG.fst)
 * Reads lang_dir/{L_disambig.fst,G.fst,words.txt,phones/disambig.int} and model_dir/{tree,final.mdl}; writes
 * graph_dir/{HCLG.fst,words.txt,disambig_tid.int,phones/...}.  dump_dir (may be NULL): LG.fst, CLG.fst, ilabels, Ha.fst and
 * HCLGa.fst are written there as well.  The result is the same weighted transducer as the reference chain's (equal weights for
 * every input / output label sequence up to the 1/1024 quantisation both apply), with this library's own state numbering. */
int rs_mkgraph(const char *lang_dir, const char *model_dir, const char *graph_dir, float transition_scale, float self_loop_scale,
               const char *dump_dir);
/* One step of that chain on files, named like the Kaldi / OpenFst executable it stands for: fsttablecompose (in1, in2 -> out),
 * fstdeterminizestar (param != 0: --use-log=true), fstminimizeencoded, fstpushspecial, fstrmepslocal, fstrmsymbols (aux = symbol
 * list), fstarcsort (aux = "ilabel" | "olabel"), fstcomposecontext (in2 = disambig list, aux = ilabels output, param = 16 * N + P),
 * make-h-transducer (in1 = ilabels, in2 = tree, aux = final.mdl, param = transition scale; the disambiguation transition-ids go to
 * out + ".disambig"), add-self-loops (aux = final.mdl, param = self-loop scale; --reorder=true), and two checks that fail with a
 * description of the first difference: fstisomorphic (same transducer up to state numbering, weights within param) and
 * fstequivalent (fstequivalent --random=true: equal tropical weight, within param, of the label pairs of random paths). */
int rs_fst_tool(const char *tool, const char *in1, const char *in2, const char *out, const char *aux, float param);

/* ---- what the reference's decoder binaries do to a model before the first frame (host side; no device needed).
 * Both binaries (kaldi/src/online2bin/online2-wav-nnet3-latgen-faster.cc:160-176, online2-cli-nnet3-decode-faster.cc:97-111)
 * run CollapseModel on the network they read and, while computing the network's context and compiling its looped computation,
 * call glibc's rand() a model-dependent number of times -- which decides the noise Dither() adds to every frame afterwards
 * (kaldi/src/feat/feature-window.cc:90-98; the default mfcc and fbank configurations have --dither=1 and rhasspy starts one process per
 * utterance, so the noise of frame t is a constant of the model).  rs_model_load replays both; these two entry points expose
 * the replay for inspection and tests:
 *   rs_nnet3_setup: *rand_calls = number of rand() calls before the first frame for `final_mdl` under --frames-per-chunk;
 *     *certain = 0 when the count assumes a looped compilation the reference may have to retry, and for every recurrent network
 *     (its compilation has another step structure, whose draws are not replayed; the context search, the collapser and the
 *     five-request walk run all the same and give the reference's context and collapsed network) (rs_model_load refuses such a
 *     model unless its mfcc.conf / fbank.conf says --dither=0); collapsed_config (may be NULL) receives the config lines of the collapsed
 *     network, '\n'-separated and NUL-terminated, truncated to buf_len.
 *   rs_dither_noise: out[(t - t0) * window + i] = the value Dither() adds, for --dither=1, to sample i of frame t in a process
 *     that called rand() `rand_calls` times before its first frame. */
int rs_nnet3_setup(const char *final_mdl, int32_t frames_per_chunk, int64_t *rand_calls, int32_t *certain, char *collapsed_config,
                   size_t buf_len);
/*   rs_nnet3_setup_subsampled: the same under --frame-subsampling-factor (the looped computation is compiled for the output frames
 *     t = 0, f, 2 f, ... and a chunk rounded up to a multiple of f: nnet-compile-looped.cc:81-94,111-128). */
int rs_nnet3_setup_subsampled(const char *final_mdl, int32_t frames_per_chunk, int32_t frame_subsampling_factor, int64_t *rand_calls,
                              int32_t *certain, char *collapsed_config, size_t buf_len);
int rs_dither_noise(int64_t rand_calls, int32_t t0, int32_t t1, int32_t window, float *out);

/* ---- rescoring against a NEW language directory (host side; the lattices come from decodes with rs_decode_opts.emit_lattice = 1).
 * Replaces the tool chain of `async_transcribe_rescore` (rhasspy_speech/transcribe_wav.py:107-232, transcribe_stream.py:131-274):
 *   [Ldet.fst from L_disambig.fst: fstprint | awk | fstcompile | fstdeterminizestar | fstrmsymbols]   lattice-scale --lm-scale=0.0 |
 *   lattice-to-phone-lattice | lattice-compose - Ldet.fst | lattice-determinize | lattice-compose --phi-label=#0 - G.fst |
 *   lattice-add-trans-probs --transition-scale=1.0 --self-loop-scale=0.1 | lattice-to-nbest --n --acoustic-scale | nbest-to-linear
 * rs_rescorer_open reads <new_lang_dir>/{L_disambig.fst, G.fst, words.txt, phones/disambig.int} once (the reference rebuilds
 * Ldet.fst and re-reads everything per utterance); it fails like the reference when words.txt has no #0. */
typedef struct rs_rescorer rs_rescorer;
int rs_rescorer_open(const rs_model *model, const char *new_lang_dir, rs_rescorer **out);
/* Rescores utterance `utt` of a result; renders the bytes `nbest-to-linear ... ark,t:-` prints at the end of the chain
 * ("<key>-<k> id id ... \n", ids of the NEW words.txt; nothing when no path survives) into buf, returns the number of bytes
 * needed (like snprintf) or a negative status.  graph_cost / acoustic_cost (may be null): up to `nbest` entries, the 4th / 5th
 * outputs of nbest-to-linear; *n_out = number of hypotheses. */
int rs_rescore_result(const rs_rescorer *r, const rs_result *res, int32_t utt, int32_t nbest, float acoustic_scale, const char *key,
                      char *buf, size_t len, float *graph_cost, float *acoustic_cost, int32_t *n_out);
/* Same on a lattice given as one binary CompactLattice table entry (what online2-wav-nnet3-latgen-faster writes, and what
 * rs_result_lattice renders): no GPU involved -- for tools and for the host-only parity tests against the reference's chain. */
int rs_rescore_lattice(const rs_rescorer *r, const char *lattice_entry, size_t n_bytes, int32_t nbest, float acoustic_scale, const char *key,
                       char *buf, size_t len, float *graph_cost, float *acoustic_cost, int32_t *n_out);
void rs_rescorer_free(rs_rescorer *r);

/* Host-side entry for tests and tools (no GPU needed): determinises a raw lattice -- the state-level lattice the search
 * leaves behind, given as n_arcs arcs (src, dst, word label, transition-id; graph and acoustic cost), a start state and
 * per-state final costs (+inf = not final) -- with the same code rs_result_lattice uses (lattice beam `beam`) and renders
 * the binary CompactLattice table entry.  Returns the entry's size (copies min(size, cap) bytes), or a negative error. */
int64_t rs_lattice_entry_from_raw(int32_t num_states, int32_t start, const float *final_cost, int32_t n_arcs, const int32_t *arc_src,
                                  const int32_t *arc_dst, const int32_t *arc_word, const int32_t *arc_tid, const float *arc_graph,
                                  const float *arc_acoustic, float beam, const char *key, char *buf, int64_t cap);

/* Host-side entries for tests and tools (no GPU needed): what results with rs_decode_opts.emit_alignment carry, from the same code.
 * rs_lattice_nbest_alignments_from_raw: the n-best word sequences of a raw lattice (given as for rs_lattice_entry_from_raw) with the
 *   costs and the transition-ids of the best alignment of each, best first.  *n_out = hypotheses found (<= nbest); hypothesis k has
 *   words word_buf[word_off[k] .. word_off[k + 1]) and transition-ids tid_buf[tid_off[k] .. tid_off[k + 1]) (the offset arrays hold
 *   nbest + 1 entries; the offsets are always the true ones, ids beyond word_cap / tid_cap are not written -- RS_ERR_ARG then);
 *   graph_cost / acoustic_cost: nbest entries, may be null.
 * rs_alignment_phones: rs_result_phones' splitting of a transition-id sequence, with the transition model of `final_mdl`; *n_out =
 *   segments (all of them counted, at most cap written). */
int rs_lattice_nbest_alignments_from_raw(int32_t num_states, int32_t start, const float *final_cost, int32_t n_arcs, const int32_t *arc_src,
                                         const int32_t *arc_dst, const int32_t *arc_word, const int32_t *arc_tid, const float *arc_graph,
                                         const float *arc_acoustic, float beam, int32_t nbest, float acoustic_scale, int32_t *n_out,
                                         int32_t *word_off, int32_t *word_buf, int32_t word_cap, int32_t *tid_off, int32_t *tid_buf, int32_t tid_cap,
                                         float *graph_cost, float *acoustic_cost);
int rs_alignment_phones(const char *final_mdl, const int32_t *tids, int32_t n_tids, int32_t *phone, int32_t *start_frame, int32_t *num_frames,
                        int32_t cap, int32_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* RHASSPY_SPEECH_HIP_H_ */
