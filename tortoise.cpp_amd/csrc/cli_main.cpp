// `tortoise` command line — the reference's CLI surface on top of the C ABI.
//
// Same flags, defaults, relative paths and exit codes as main() in /root/reference/main.cpp:6528-6584:
//   --message <str>   default "this is a test message."
//   --voice <path>    default ../models/mol.bin        (1024 raw f32 auto_conditioning)
//   --output <path>   default ./output.wav             (24 kHz mono IEEE-float WAV)
//   --seed <int>      std::stoi -> mt19937::seed; absent => wall-clock ms
// Flags are matched as adjacent pairs at argv[i], i < argc-1; unknown flags are ignored.
// Weights are read from ../models/ggml-model.bin, ggml-diffusion-model.bin, ggml-vocoder-model.bin
// and the tokenizer from ../models/tokenizer.json (main.cpp:5078, 5625, 6046, 6551).
// Extensions (not in the reference): --models <dir>, --candidates <n> (all candidates are carried
// through; candidate 0 is written to --output like the reference, others to <output>.<c>.wav),
// --steps <n> diffusion steps (default 80), --device <ordinal>, --codes <n>,
// --clvp <file>: re-rank the candidates with CLVP (not in the reference, which keeps candidate 0, main.cpp:6575; upstream tortoise-tts
//   does this): every candidate's codes are scored against the text, only the best one goes through diffusion + vocoder and is written
//   to --output. With --devices every worker scores its own shard and the parent keeps the best of the workers' winners.
// --diffusion-latent <file>: 2048 raw f32 that replace the `diffusion_conditioning_latent` weight of ggml-diffusion-model.bin (the reference
//   bakes ONE voice into that file, main.cpp:1557-1560); with --voice this makes a voice two small files (tools/make_voice.py writes both).
// --devices <N> [--device-map a,b,...]: candidate-parallel multi-GPU run. The process re-executes itself once per GPU
//   (one process per device, replicated weights); worker r takes candidates [r B/N, (r+1) B/N) of the ONE batch: the RNG stream
//   partition (options rng_shard_offset / rng_shard_total) makes the N x B/N codes identical to a single-GPU run of B candidates,
//   device noise is keyed by the global candidate id, and the throughput stop rule (TTS_AR_RETIRE) needs no per-step exchange.
//   --exchange files (default): nothing is exchanged between workers — candidates never interact — each writes its own candidates' WAV
//   files (<output> for candidate 0, <output>.<c>.wav for the others, c = global candidate index).
//   --exchange rccl: the workers form one RCCL communicator (cli_rccl.h; distinct GPUs per worker): rank 0 broadcasts the conditioning
//   (text ids + voice latent), the result sizes / CLVP scores are all-gathered, the audio is sent to rank 0, which writes every WAV file.
// --split-text <N> (0 = off, the default): a message longer than one prompt. It is split into chunks of at most N text ids (tts_split_text: whole sentences
//   packed greedily, include/tortoise_mi355x.h states the rule); all chunks run through ONE tts_autoregressive_multi call (--candidates per chunk), each
//   chunk keeps candidate 0 (or the CLVP best with --clvp), one tts_diffusion and one tts_vocoder call run over the kept candidates, and their audio is
//   written to --output one after the other as ONE file. A message that fits one chunk takes the path without the flag. Not with --devices > 1.
// Several speakers: --voice (and --diffusion-latent) may be repeated, the k-th occurrence is voice k; one occurrence is the behaviour above. With more than one
//   --voice the message is a dialogue (tts_split_turns: one turn per line, "<index>|" in front of a turn names its voice, a turn without it keeps the voice of the
//   turn before, the first defaults to voice 0; --split-text N = ids per chunk inside a turn, default 404). Every chunk is a prompt group with its voice in ONE
//   tts_autoregressive_multi_voice call (--candidates per chunk, --clvp per chunk), the kept candidates run through one tts_diffusion_multi_voice and one
//   tts_vocoder call and their audio is written to --output in message order as ONE file. --diffusion-latent: none (every speaker uses the model's own latent)
//   or one per --voice; anything else is a usage error (exit 1) before a model is loaded. Not with --devices > 1: the conditioning broadcast carries one voice.
//   --dry-run 1 prints one line per chunk ("chunk k: voice v, n text ids") and exits 0.
// --sampler ddpm|ddim|dpmpp2m (default ddpm = the reference's ancestral loop; ddim = upstream tortoise-tts' ddim_sample; dpmpp2m = DPM-Solver++(2M), the second-order
//   multistep solver of upstream's fast presets, deterministic: --ddim-eta is checked and not read; option diff_sampler), --ddim-eta <x> (0 .. 1, default 0 =
//   deterministic) and --cond-free-k <x> (guidance strength, default 2.0): the diffusion sampler behind --steps, which keeps its meaning. Another sampler name or a value
//   out of range is a usage error (exit 1) before a model is loaded or a worker started. --devices N workers receive the flags with the rest of the command line;
//   --timing 1 echoes them ("[timing] sampler ...", one line per process).
// --cond-free 0|1 (default 1 = guided; 0 = unguided: the unconditioned branch is not evaluated, half the rows per step; option cond_free = upstream's cond_free) and
//   --diffusion-temperature <x> (finite, >= 0, default 1: x_T = x * z_T; option diff_temperature = upstream's diffusion_temperature), under the same rules: another
//   value is a usage error, workers receive them, --timing 1 echoes them on a line of their own ("[timing] cond-free ...").
// --temperature <x> (> 0, default 0.8), --top-k <n> (1 .. 8194, default 50), --top-p <x> (0 < x <= 1, default 0.8), --repetition-penalty <x> (>= 1, default 2.0) and
//   --penalty-scope last|history (default last = the reference: the ids of the last input; history = upstream's HF generate: every code sampled so far): the
//   autoregressive sampler (options ar_temperature, ar_top_k, ar_top_p, ar_repetition_penalty, ar_penalty_scope). A value out of range or another scope name is a usage
//   error (exit 1) before a model is loaded or a worker started; an absent flag leaves the engine option alone. --devices N workers receive the flags with the rest
//   of the command line; --timing 1 echoes them ("[timing] ar sampler ...").
// --typical-mass <x> (0 = off, the default; 0 < x < 1): locally typical sampling (option ar_typical_mass; upstream's typical_sampling / typical_mass), under the
//   same rules: out of range is a usage error; given, the value is appended to the "[timing] ar sampler" line.
// --decoder diffusion|hifigan (default diffusion = the reference's 80 diffusion steps + UnivNet): hifigan sends the kept candidates' latents and their voices through ONE
//   tts_hifigan_decode call (upstream tortoise-tts' api_fast.py path: no diffusion, no noise, no vocoder) and writes 256 samples per frame. --hifigan-model <file>
//   (default <models>/ggml-hifigan-model.bin); the diffusion and vocoder models are then neither loaded nor required. --clvp, --split-text and several --voice work
//   as with the diffusion decoder. Usage errors (exit 1, before a model is loaded): another decoder name; with hifigan any of --steps, --sampler, --ddim-eta,
//   --cond-free-k, --cond-free, --diffusion-temperature, --diffusion-latent (they configure the decoder that is not run), --devices > 1 or --exchange rccl. --timing 1 names the decoder ("[timing] decoder ...").
// --vocoder univnet|bigvgan (default univnet = the reference's vocoder): bigvgan sends the diffusion stage's mel through ONE tts_bigvgan call (NVIDIA BigVGAN v1, the
//   vocoder the tortoise forks put in UnivNet's place: no noise is drawn) and writes 256 samples per frame. --bigvgan-model <file> (default
//   <models>/ggml-bigvgan-model.bin); the UnivNet model is then neither loaded nor required. --clvp, --cvvp, --split-text, several --voice and every sampler flag
//   work unchanged. Usage errors (exit 1, before a model is loaded): another vocoder name; bigvgan with --decoder hifigan, --devices > 1 or --exchange rccl.
//   --timing 1 names the vocoder ("[timing] vocoder ...").
// --stream (with --decoder hifigan; no value) [--stream-stride N, default 16]: one candidate through tts_hifigan_stream. The samples are appended to the WAV as the
//   callback receives them, while the autoregressive stage is still sampling, and the header's two sizes are fixed at the end: the file is byte for byte the one the
//   run without --stream writes. --timing 1 prints when the first samples arrived ("[timing] first audio ..."), from the start of the process and from the start of the
//   autoregressive stage. Usage errors (exit 1, before a model is loaded): --stream with --decoder diffusion, --clvp, --split-text, several --voice, --candidates > 1
//   or --devices > 1; --stream-stride < 1.
// --voice-clips a.wav[,b.wav...] --conditioning-model F --diffusion-conditioning-model G [--mel-norms F] [--save-voice PREFIX]: a voice made from audio clips on
//   the device (tts_voice_from_audio: RIFF WAV with PCM16, PCM24 or float32 samples at any rate; upstream's resampling, windows and mels). Every occurrence of
//   --voice-clips is ONE voice made from its comma-separated clips; the voices are numbered in command-line order together with the --voice occurrences and work
//   with the "<index>|" turns and with --decoder hifigan like them. F / G: the two encoder files (tools/convert_weights.py --conditioning-encoder /
//   --diffusion-conditioning-encoder); with --decoder hifigan G is optional (without it no diffusion latent is made). --mel-norms: 80 raw f32, upstream's
//   data/mel_norms.pth. --save-voice PREFIX (none, or one per --voice-clips, in order) writes PREFIX.bin and, when G is given, PREFIX.diffusion.bin: the files
//   --voice and --diffusion-latent read. With the diffusion decoder a clip voice brings its own diffusion latent, so every --voice beside it needs its
//   --diffusion-latent. Usage errors (exit 1, before a model is loaded): a missing encoder file, --dry-run 1, --devices > 1 or --exchange rccl, a wrong count of
//   --save-voice or --diffusion-latent.
// --voice-random SEED --random-voice-model F [--random-diffusion-voice-model G] [--save-voice PREFIX]: a random voice, what upstream's do_tts.py --voice random (its
//   default) and tts() without clips or latents produce: RandomLatentConverter on the device (tts_load_random_voice / tts_random_voice; not in the reference),
//   its input drawn from the device generator under SEED, an unsigned 64-bit integer; --seed and the sampler's generator are not involved. Every occurrence of
//   --voice-random is ONE voice, numbered in command-line order together with the --voice and --voice-clips occurrences, and works with the "<index>|" turns.
//   F / G: the two model files (tools/convert_weights.py --random-voice / --random-diffusion-voice); G is required with the diffusion decoder and optional with
//   --decoder hifigan. As a clip voice, a random voice brings its own diffusion latent, so every --voice file beside it needs its --diffusion-latent.
//   --save-voice PREFIX (none, or one per --voice-clips and --voice-random together, in command-line order) writes PREFIX.bin and, when the diffusion latent was
//   made, PREFIX.diffusion.bin: the run with --voice PREFIX.bin --diffusion-latent PREFIX.diffusion.bin and the same --seed writes the same WAV bytes. A literal
//   --voice random keeps meaning a file named `random`. Usage errors (exit 1, before a model is loaded): a missing model file, --dry-run 1, --devices > 1 or
//   --exchange rccl, a wrong count of --save-voice or --diffusion-latent, a SEED that is not an unsigned 64-bit integer.
// --cvvp <file> [--cvvp-amount x]: re-rank the candidates with CVVP as well (tts_load_cvvp: do these codes sound like this speaker?; not in the reference): every
//   candidate's codes are scored against the clips of its voice, one conditioning latent per clip made once per voice (tts_cvvp_voice_audio with --mel-norms), and
//   the candidate with the best clvp * (1 - x) + cvvp * x is kept, upstream's cvvp_amount. x defaults to 0.5 beside --clvp and to 1 without it; the side whose
//   weight is 0 is neither loaded nor evaluated, so --cvvp-amount 0 is the run without --cvvp, byte for byte. Prints "cvvp scores:" beside "clvp scores:" (per chunk
//   with --split-text or several voices, where every chunk is scored against its own voice's clips). Usage errors (exit 1, before a model is loaded): a voice
//   given as a --voice latent file, which holds no audio (the default voice is one); --devices > 1 or --exchange rccl; --stream; x outside 0 .. 1; 0 < x < 1
//   without --clvp; --cvvp-amount without --cvvp.
// --detect a.wav[,b.wav...] --classifier FILE: tortoise-detect, the classifier upstream ships beside the generator (tts_load_classifier / tts_classify_audio; not in
//   the reference). Prints one line per clip, "detect: <path> <probability that the clip is Tortoise's>", and exits; no other model is loaded or required. On a
//   synthesis run --classifier FILE scores the WAV the run has just written and prints "classifier: <path> <probability>" on stderr. Usage errors (exit 1,
//   before a model is loaded): --detect without --classifier, either with --dry-run 1, --classifier with --devices > 1 or --exchange rccl.
// --aligner FILE: redact bracketed prompt text, as upstream's Wav2VecAlignment.redact does (tts_load_aligner / tts_redact_audio; not in the reference). In
//   "[I am so sad,] the package never came." the bracketed words steer the delivery but are not heard: with the flag '[' and ']' are removed from the message
//   before it is tokenised (the words are spoken), and the audio of the bracketed parts is cut out of the chosen candidate before --output is written. A message
//   without brackets, or a run without --aligner (brackets or not), writes the bytes it wrote before. A failed alignment ("the text does not match the audio")
//   exits 1 and writes no WAV. Usage errors (exit 1, before a model is loaded), for --aligner with a bracketed message only: --split-text, several voices,
//   --stream, --devices > 1 or --exchange rccl, --dry-run 1; unbalanced or nested brackets.
// --dvae FILE: the DVAE encoder, speech codes from audio (tts_load_dvae / tts_dvae_codes_audio; not in the reference). --mel-norms FILE gives the AR side's
//   per-band norms, as with --voice-clips.
//   --codes-from a.wav[,b.wav...] [--codes-out FILE]: prints "codes: <path> c0 c1 ..." per clip, or writes one line of space-separated codes per clip to FILE,
//   and exits; no other model is loaded or required and nothing is synthesised.
//   --revoice in.wav --message "transcript": the recording's codes under its transcript and the chosen voice (tts_ar_latents_for_codes: no sampling), then the
//   chosen decoder chain (diffusion + vocoder, or --decoder hifigan) -> --output: the recording re-spoken in the other voice. Every voice option works as before.
//   Usage errors (exit 1, before a model is loaded): --codes-from or --revoice without --dvae, either with --dry-run 1, --revoice with --split-text,
//   --candidates > 1, several voices, --stream, --clvp / --cvvp, --devices > 1 or --exchange rccl, an unreadable clip, or a clip of more than 500 codes.
// --score-audio a.wav[,b.wav...] (with --dvae FILE) or --score-codes FILE (lines in --codes-out's format), with --message "transcript", any voice source and the
//   AR model: teacher-forced scores of the clips' codes under the transcript and the voice (tts_ar_score_codes: one batched pass, no sampling; nothing is
//   synthesised and no other model is loaded). [--score-positions decode|train], default train (upstream forward()'s positions; decode = what the sampler saw).
//   Per clip one line "score: <path or FILE:line> <codes n> <total log-likelihood of the n codes and the stop> <mean negative log-likelihood in nats per scored
//   position, n + 1 of them> <perplexity = exp of that> <the stop token's log-prob at the last position> <share of positions whose argmax is the target>".
//   Usage errors (exit 1, before a model is loaded): both options at once, --score-audio without --dvae, no --message, --dry-run 1, --score-positions without
//   either or with another word, a combination with --revoice, --codes-from, --split-text, --stream, several voices, --devices > 1 or --exchange rccl, an
//   unreadable clip or codes file, a line that is not 1 .. 500 codes in 0 .. 8191, more than 64 clips, a clip of more than 500 codes (chunking is the caller's).
#include "tortoise_mi355x.h"
#include "cli_rccl.h"
#include <algorithm>
#include <cmath>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cerrno>
#include <cctype>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <string>
#include <vector>
#include <sys/wait.h>
#include <unistd.h>
#include <chrono>
#include <thread>

// --stream: the callback of tts_hifigan_stream appends the samples to the open WAV
struct StreamSink {
  FILE *f = nullptr;
  int64_t samples = 0;
  int calls = 0;
  bool failed = false;
  std::chrono::steady_clock::time_point t_ar, t_first;
  static int on_audio(void *user, const float *s, int n, int /*is_last*/) {
    StreamSink *k = (StreamSink *)user;
    if (k->calls++ == 0) k->t_first = std::chrono::steady_clock::now();
    if (fwrite(s, sizeof(float), (size_t)n, k->f) != (size_t)n || fflush(k->f)) { k->failed = true; return 1; }
    k->samples += n;
    return 0;
  }
};

// one WAV file (mono mix, any rate) appended to `samples`; false with a message on stderr
static bool read_clip(const std::string &path, std::vector<float> &samples, int64_t *n, int32_t *rate) {
  const int64_t cnt = tts_read_wav(path.c_str(), nullptr, 0, rate);
  if (cnt < 1) { fprintf(stderr, "%s: not a readable RIFF WAV with PCM16, PCM24 or float32 samples\n", path.c_str()); return false; }
  samples.resize(samples.size() + (size_t)cnt);
  if (tts_read_wav(path.c_str(), samples.data() + samples.size() - (size_t)cnt, cnt, rate) != cnt) { fprintf(stderr, "%s: read error\n", path.c_str()); return false; }
  *n = cnt;
  return true;
}
// codes a clip of n samples at `rate` Hz gives the DVAE under upstream's configuration: the mel of the whole clip at 22 050 Hz, hop 256
static int clip_codes(int64_t n, int rate) { return tts_dvae_rows((int)((n * 22050 + rate - 1) / rate / 256) + 1); }
// --mel-norms FILE: 80 floats, or none
static bool read_norms(const std::string &path, std::vector<float> &norms) {
  if (path.empty()) return true;
  norms.resize(80);
  std::ifstream f(path, std::ios::binary);
  if (!f || !f.read((char *)norms.data(), 80 * sizeof(float))) { std::cerr << "Error: Unable to read 80 floats from " << path << std::endl; return false; }
  return true;
}

// the clips of a comma-separated list of WAV files (mono mix, any rate) through ONE tts_classify_audio call; prob: one value per clip
static int classify_wavs(tts_ctx *ctx, const std::string &list, std::vector<std::string> &paths, std::vector<float> &prob) {
  std::vector<float> samples;
  std::vector<int64_t> ns;
  std::vector<int32_t> rates;
  for (size_t a = 0; a <= list.size();) {
    const size_t b = std::min(list.find(',', a), list.size());
    const std::string path = list.substr(a, b - a);
    a = b + 1;
    if (path.empty()) continue;
    int32_t rate = 0;
    const int64_t cnt = tts_read_wav(path.c_str(), nullptr, 0, &rate);
    if (cnt < 1) { fprintf(stderr, "%s: not a readable RIFF WAV with PCM16, PCM24 or float32 samples\n", path.c_str()); return 1; }
    samples.resize(samples.size() + (size_t)cnt);
    if (tts_read_wav(path.c_str(), samples.data() + samples.size() - (size_t)cnt, cnt, &rate) != cnt) { fprintf(stderr, "%s: read error\n", path.c_str()); return 1; }
    paths.push_back(path); ns.push_back(cnt); rates.push_back(rate);
  }
  if (paths.empty()) { fprintf(stderr, "--detect: no clip given\n"); return 1; }
  prob.assign(paths.size(), 0.f);
  if (tts_classify_audio(ctx, samples.data(), ns.data(), rates.data(), (int)paths.size(), prob.data(), nullptr)) {
    fprintf(stderr, "classify_audio: %s\n", tts_last_error(ctx));
    return 1;
  }
  return 0;
}

static int die(tts_ctx *c, const char *what) {
  fprintf(stderr, "%s: %s\n", what, tts_last_error(c));
  return 1; // the reference exit(1)s on load failure (main.cpp:5089, 5634, 6069)
}

int main(int argc, char **argv) {
  std::string message = "this is a test message.";
  std::string voicePath = "../models/mol.bin";
  std::string outputPath = "./output.wav";
  std::string modelsDir = "../models";
  bool have_seed = false;
  int seed = 0, candidates = 1, steps = 80, device = 0, fixed_codes = 0, devices = 1, shard = -1, nshards = 1, split_ids = 0;
  std::string device_map, clvpPath, exchange = "files", rccl_id, diffLatentPath;
  std::string cvvpPath;
  double cvvp_amount = 0.0;
  bool have_cvvp_amount = false;
  bool dry = false, allow_shared = false;
  bool timing = false;
  int test_fail_shard = -1, test_slow_shard = -1;
  std::vector<std::pair<std::string, double>> engine_options; // --option key=value (repeatable): tts_set_option before the models are loaded
  std::string sampler = "ddpm";
  double ddim_eta = 0.0, cond_free_k = 2.0;
  std::string cond_free = "1";
  double diff_temp = 1.0;
  bool have_cond_free = false, have_diff_temp = false;
  bool have_sampler = false, have_eta = false, have_k = false; // a flag that is absent leaves the engine's option (default, or --option) alone
  double ar_temp = 0.8, ar_top_k = 50, ar_top_p = 0.8, ar_pen = 2.0; // the autoregressive sampler's controls, same rule
  std::string ar_scope = "last";
  double ar_typ = 0;
  bool have_typ = false;
  std::string decoder = "diffusion", hifiganPath, vocoder = "univnet", bigvganPath;
  std::string detectClips, classifierPath, alignerPath;
  std::string dvaePath, codesFrom, codesOut, revoicePath, scoreAudio, scoreCodes, scorePositions;
  bool have_steps = false;
  bool have_temp = false, have_top_k = false, have_top_p = false, have_pen = false, have_scope = false;
  std::vector<std::string> voicePaths, diffLatentPaths;        // every occurrence of --voice / --diffusion-latent: the k-th is voice k
  std::vector<std::string> voiceRandom;                        // parallel to voicePaths: "R" + the SEED text of a --voice-random voice ("" for every other voice)
  std::string rlgModel, rlgDiffModel;                          // --random-voice-model / --random-diffusion-voice-model
  std::vector<std::string> voiceClips, saveVoice;              // parallel to voicePaths: the clip list of a --voice-clips voice ("" for a --voice file); --save-voice prefixes
  std::string condModel, dcondModel, melNormsPath;
  bool stream = false;
  int stream_stride = 16;
  StreamSink sink;
  for (int i = 1; i < argc; ++i) { // --stream is the one flag without a value: every other "--flag" owns the slot after it, which is not looked at here
    const std::string a(argv[i]);
    if (a == "--stream") stream = true;
    else if (a.rfind("--", 0) == 0) ++i;
  }
  for (int i = 1; i < argc - 1; ++i) {
    std::string a(argv[i]);
    if (a == "--stream-stride") stream_stride = std::stoi(argv[i + 1]);
    else if (a == "--voice") { voicePath = argv[i + 1]; voicePaths.push_back(voicePath); voiceClips.push_back(""); voiceRandom.push_back(""); }
    else if (a == "--voice-clips") { voicePath.clear(); voicePaths.push_back(""); voiceClips.push_back(argv[i + 1]); voiceRandom.push_back(""); }
    else if (a == "--voice-random") { voicePath.clear(); voicePaths.push_back(""); voiceClips.push_back(""); voiceRandom.push_back(std::string("R") + argv[i + 1]); }
    else if (a == "--random-voice-model") rlgModel = argv[i + 1];
    else if (a == "--random-diffusion-voice-model") rlgDiffModel = argv[i + 1];
    else if (a == "--conditioning-model") condModel = argv[i + 1];
    else if (a == "--diffusion-conditioning-model") dcondModel = argv[i + 1];
    else if (a == "--mel-norms") melNormsPath = argv[i + 1];
    else if (a == "--save-voice") saveVoice.push_back(argv[i + 1]);
    else if (a == "--message") message = argv[i + 1];
    else if (a == "--output") outputPath = argv[i + 1];
    else if (a == "--seed") { seed = std::stoi(argv[i + 1]); have_seed = true; }
    else if (a == "--models") modelsDir = argv[i + 1];
    else if (a == "--candidates") candidates = std::stoi(argv[i + 1]);
    else if (a == "--steps") { steps = std::stoi(argv[i + 1]); have_steps = true; }
    else if (a == "--decoder") decoder = argv[i + 1];
    else if (a == "--hifigan-model") hifiganPath = argv[i + 1];
    else if (a == "--vocoder") vocoder = argv[i + 1];
    else if (a == "--bigvgan-model") bigvganPath = argv[i + 1];
    else if (a == "--detect") detectClips = argv[i + 1];
    else if (a == "--classifier") classifierPath = argv[i + 1];
    else if (a == "--aligner") alignerPath = argv[i + 1];
    else if (a == "--dvae") dvaePath = argv[i + 1];
    else if (a == "--codes-from") codesFrom = argv[i + 1];
    else if (a == "--codes-out") codesOut = argv[i + 1];
    else if (a == "--revoice") revoicePath = argv[i + 1];
    else if (a == "--score-audio") scoreAudio = argv[i + 1];
    else if (a == "--score-codes") scoreCodes = argv[i + 1];
    else if (a == "--score-positions") scorePositions = argv[i + 1];
    else if (a == "--device") device = std::stoi(argv[i + 1]);
    else if (a == "--codes") fixed_codes = std::stoi(argv[i + 1]); // exactly N sampled codes, stop token masked (synthetic weights never stop)
    else if (a == "--devices") devices = std::stoi(argv[i + 1]);
    else if (a == "--device-map") device_map = argv[i + 1];
    else if (a == "--allow-shared-device") allow_shared = argv[i + 1][0] != '0';
    else if (a == "--clvp") clvpPath = argv[i + 1];
    else if (a == "--cvvp") cvvpPath = argv[i + 1];
    else if (a == "--cvvp-amount") { cvvp_amount = std::atof(argv[i + 1]); have_cvvp_amount = true; }
    else if (a == "--exchange") exchange = argv[i + 1];
    else if (a == "--dry-run") dry = argv[i + 1][0] != '0'; // plumbing check without a device, see below
    else if (a == "--timing") timing = argv[i + 1][0] != '0'; // wall clock of every phase of this process on stderr
    else if (a == "--test-fail-shard") test_fail_shard = std::stoi(argv[i + 1]); // test hooks (tests/test_distributed_cpu.py): worker r exits with status 3 after the
    else if (a == "--test-slow-shard") test_slow_shard = std::stoi(argv[i + 1]); // conditioning broadcast / sleeps 2 s before the final exchange
    else if (a == "--option") { // engine option, e.g. --option attn_f32=1 (include/tortoise_mi355x.h: tts_set_option)
      const std::string kv = argv[i + 1];
      const size_t eq = kv.find('=');
      if (eq == std::string::npos) { fprintf(stderr, "--option %s: expected key=value\n", kv.c_str()); return 1; }
      engine_options.emplace_back(kv.substr(0, eq), std::atof(kv.c_str() + eq + 1));
    }
    else if (a == "--diffusion-latent") { diffLatentPath = argv[i + 1]; diffLatentPaths.push_back(diffLatentPath); }
    else if (a == "--split-text") split_ids = std::stoi(argv[i + 1]);
    else if (a == "--sampler") { sampler = argv[i + 1]; have_sampler = true; }
    else if (a == "--ddim-eta") { ddim_eta = std::atof(argv[i + 1]); have_eta = true; }
    else if (a == "--cond-free-k") { cond_free_k = std::atof(argv[i + 1]); have_k = true; }
    else if (a == "--cond-free") { cond_free = argv[i + 1]; have_cond_free = true; }
    else if (a == "--diffusion-temperature") { diff_temp = std::atof(argv[i + 1]); have_diff_temp = true; }
    else if (a == "--temperature") { ar_temp = std::atof(argv[i + 1]); have_temp = true; }
    else if (a == "--top-k") { ar_top_k = std::atof(argv[i + 1]); have_top_k = true; }
    else if (a == "--top-p") { ar_top_p = std::atof(argv[i + 1]); have_top_p = true; }
    else if (a == "--repetition-penalty") { ar_pen = std::atof(argv[i + 1]); have_pen = true; }
    else if (a == "--typical-mass") { ar_typ = std::atof(argv[i + 1]); have_typ = true; }
    else if (a == "--penalty-scope") { ar_scope = argv[i + 1]; have_scope = true; }
    else if (a == "--rccl-id") rccl_id = argv[i + 1]; // worker mode (set by the parent)
    else if (a == "--shard") { // worker mode (set by the parent): "r/N"
      std::string v(argv[i + 1]);
      const size_t sl = v.find('/');
      if (sl != std::string::npos) { shard = std::stoi(v.substr(0, sl)); nshards = std::stoi(v.substr(sl + 1)); }
    }
  }
  if (exchange != "files" && exchange != "rccl") { fprintf(stderr, "--exchange %s: files or rccl\n", exchange.c_str()); return 1; }
  if (decoder != "diffusion" && decoder != "hifigan") { fprintf(stderr, "--decoder %s: diffusion or hifigan\n", decoder.c_str()); return 1; }
  const bool use_hifigan = decoder == "hifigan";
  if (use_hifigan) {
    const char *bad = have_steps ? "--steps" : have_sampler ? "--sampler" : have_eta ? "--ddim-eta" : have_k ? "--cond-free-k" : have_cond_free ? "--cond-free" : have_diff_temp ? "--diffusion-temperature" : !diffLatentPaths.empty() ? "--diffusion-latent" : nullptr;
    if (bad) { fprintf(stderr, "%s configures the diffusion decoder, which --decoder hifigan does not run\n", bad); return 1; }
    if (devices > 1 || exchange == "rccl" || shard >= 0) { fprintf(stderr, "--decoder hifigan cannot be combined with --devices > 1 or --exchange rccl\n"); return 1; }
  }
  if (vocoder != "univnet" && vocoder != "bigvgan") { fprintf(stderr, "--vocoder %s: univnet or bigvgan\n", vocoder.c_str()); return 1; }
  const bool use_bigvgan = vocoder == "bigvgan";
  if (use_bigvgan) {
    if (use_hifigan) { fprintf(stderr, "--vocoder bigvgan reads the diffusion decoder's mel: it cannot be combined with --decoder hifigan\n"); return 1; }
    if (devices > 1 || exchange == "rccl" || shard >= 0) { fprintf(stderr, "--vocoder bigvgan cannot be combined with --devices > 1 or --exchange rccl\n"); return 1; }
  }
  if (!detectClips.empty() && classifierPath.empty()) { fprintf(stderr, "--detect needs --classifier <file> (tools/convert_weights.py --classifier)\n"); return 1; }
  if (!classifierPath.empty()) {
    if (dry) { fprintf(stderr, "--classifier runs on the device: it cannot be combined with --dry-run 1\n"); return 1; }
    if (detectClips.empty() && (devices > 1 || exchange == "rccl" || shard >= 0)) { fprintf(stderr, "--classifier cannot be combined with --devices > 1 or --exchange rccl\n"); return 1; }
  }
  if (!detectClips.empty()) { // tortoise-detect: the classifier alone
    tts_ctx *dctx = tts_create(device);
    if (!dctx) { fprintf(stderr, "tts_create(%d) failed: no HIP device (this engine has no CPU path)\n", device); return 1; }
    if (tts_load_classifier(dctx, classifierPath.c_str())) { const int rc = die(dctx, "classifier_model_load"); tts_destroy(dctx); return rc; }
    std::vector<std::string> paths;
    std::vector<float> prob;
    const int rc = classify_wavs(dctx, detectClips, paths, prob);
    for (size_t c = 0; !rc && c < paths.size(); c++) printf("detect: %s %.9g\n", paths[c].c_str(), (double)prob[c]);
    tts_destroy(dctx);
    return rc;
  }
  // --dvae: speech codes from audio
  const bool revoice = !revoicePath.empty();
  std::vector<float> rv_samples; // --revoice: the recording, read before any model is loaded (a clip over 500 codes is a usage error)
  int64_t rv_n = 0;
  int32_t rv_rate = 0;
  if ((!codesFrom.empty() || revoice) && dvaePath.empty()) {
    fprintf(stderr, "usage: %s needs --dvae <file> (tools/convert_weights.py --dvae)\n", revoice ? "--revoice" : "--codes-from");
    return 1;
  }
  if (!codesOut.empty() && codesFrom.empty()) { fprintf(stderr, "usage: --codes-out needs --codes-from <a.wav[,b.wav...]>\n"); return 1; }
  if (!dvaePath.empty() && dry) { fprintf(stderr, "usage: --dvae runs on the device: it cannot be combined with --dry-run 1\n"); return 1; }
  if (revoice) {
    const char *bad = !codesFrom.empty() ? "--codes-from" : split_ids > 0 ? "--split-text" : candidates > 1 ? "--candidates > 1" : voicePaths.size() > 1 ? "several voices" :
                      stream ? "--stream" : (!clvpPath.empty() || !cvvpPath.empty()) ? "--clvp / --cvvp" : (devices > 1 || exchange == "rccl" || shard >= 0) ? "--devices > 1 or --exchange rccl" :
                      fixed_codes > 0 ? "--codes" : nullptr;
    if (bad) { fprintf(stderr, "usage: --revoice re-speaks one recording in one voice without sampling: it cannot be combined with %s\n", bad); return 1; }
    if (message.empty()) { fprintf(stderr, "usage: --revoice needs --message \"the recording's transcript\"\n"); return 1; }
    if (!read_clip(revoicePath, rv_samples, &rv_n, &rv_rate)) return 1;
    if (clip_codes(rv_n, rv_rate) > 500) {
      fprintf(stderr, "usage: --revoice %s: %lld samples at %d Hz make %d codes, at most 500 (about 23 s; cut the recording)\n", revoicePath.c_str(), (long long)rv_n,
              rv_rate, clip_codes(rv_n, rv_rate));
      return 1;
    }
  }
  if (!codesFrom.empty()) { // the encoder alone: one tts_dvae_codes_audio call for all clips
    std::vector<float> samples, norms;
    std::vector<int64_t> ns;
    std::vector<int32_t> rates;
    std::vector<std::string> paths;
    int stride = 1;
    for (size_t a = 0; a <= codesFrom.size();) {
      const size_t b = std::min(codesFrom.find(',', a), codesFrom.size());
      const std::string path = codesFrom.substr(a, b - a);
      a = b + 1;
      if (path.empty()) continue;
      int64_t cnt = 0;
      int32_t rate = 0;
      if (!read_clip(path, samples, &cnt, &rate)) return 1;
      paths.push_back(path); ns.push_back(cnt); rates.push_back(rate);
      stride = std::max(stride, clip_codes(cnt, rate) + 1);
    }
    if (paths.empty()) { fprintf(stderr, "usage: --codes-from: no clip given\n"); return 1; }
    if (!read_norms(melNormsPath, norms)) return 1;
    tts_ctx *dctx = tts_create(device);
    if (!dctx) { fprintf(stderr, "tts_create(%d) failed: no HIP device (this engine has no CPU path)\n", device); return 1; }
    if (tts_load_dvae(dctx, dvaePath.c_str())) { const int rc = die(dctx, "dvae_model_load"); tts_destroy(dctx); return rc; }
    tts_voice_audio_opts vo;
    vo.struct_size = sizeof vo;
    tts_voice_audio_opts_init(&vo);
    vo.mel_norms80 = norms.empty() ? nullptr : norms.data();
    std::vector<int32_t> codes(paths.size() * (size_t)stride), nc(paths.size());
    if (tts_dvae_codes_audio(dctx, samples.data(), ns.data(), rates.data(), (int)paths.size(), &vo, codes.data(), nc.data(), stride, nullptr)) {
      const int rc = die(dctx, "dvae_codes_audio");
      tts_destroy(dctx);
      return rc;
    }
    tts_destroy(dctx);
    FILE *out = codesOut.empty() ? stdout : fopen(codesOut.c_str(), "w");
    if (!out) { fprintf(stderr, "--codes-out %s: cannot be opened\n", codesOut.c_str()); return 1; }
    for (size_t c = 0; c < paths.size(); c++) {
      if (codesOut.empty()) fprintf(out, "codes: %s", paths[c].c_str());
      for (int i = 0; i < nc[c]; i++) fprintf(out, i || codesOut.empty() ? " %d" : "%d", codes[c * (size_t)stride + i]);
      fprintf(out, "\n");
    }
    if (!codesOut.empty() && fclose(out)) { fprintf(stderr, "--codes-out %s: write error\n", codesOut.c_str()); return 1; }
    return 0;
  }
  // --score-audio / --score-codes: everything that can be refused is refused here, before a model is loaded
  const bool score = !scoreAudio.empty() || !scoreCodes.empty();
  std::vector<float> sc_samples;
  std::vector<int64_t> sc_ns;
  std::vector<int32_t> sc_rates, sc_codes /*[clips][500]*/, sc_n;
  std::vector<std::string> sc_names;
  if (!scorePositions.empty() && !score) { fprintf(stderr, "usage: --score-positions needs --score-audio or --score-codes\n"); return 1; }
  if (score) {
    if (!scoreAudio.empty() && !scoreCodes.empty()) { fprintf(stderr, "usage: --score-audio and --score-codes cannot be combined\n"); return 1; }
    if (!scoreAudio.empty() && dvaePath.empty()) { fprintf(stderr, "usage: --score-audio needs --dvae <file> (tools/convert_weights.py --dvae)\n"); return 1; }
    if (dry) { fprintf(stderr, "usage: --score-audio / --score-codes run on the device: they cannot be combined with --dry-run 1\n"); return 1; }
    if (!scorePositions.empty() && scorePositions != "decode" && scorePositions != "train") { fprintf(stderr, "usage: --score-positions %s: decode or train\n", scorePositions.c_str()); return 1; }
    const char *bad = revoice ? "--revoice" : split_ids > 0 ? "--split-text" : stream ? "--stream" : voicePaths.size() > 1 ? "several voices" :
                      (devices > 1 || exchange == "rccl" || shard >= 0) ? "--devices > 1 or --exchange rccl" : nullptr;
    if (bad) { fprintf(stderr, "usage: --score-audio / --score-codes score given codes under one transcript and one voice: they cannot be combined with %s\n", bad); return 1; }
    if (message.empty()) { fprintf(stderr, "usage: --score-audio / --score-codes need --message \"the transcript\"\n"); return 1; }
    if (!scoreAudio.empty()) {
      for (size_t a = 0; a <= scoreAudio.size();) {
        const size_t b = std::min(scoreAudio.find(',', a), scoreAudio.size());
        const std::string path = scoreAudio.substr(a, b - a);
        a = b + 1;
        if (path.empty()) continue;
        int64_t cnt = 0;
        int32_t rate = 0;
        if (!read_clip(path, sc_samples, &cnt, &rate)) return 1;
        if (clip_codes(cnt, rate) > 500) {
          fprintf(stderr, "usage: --score-audio %s: %lld samples at %d Hz make %d codes, at most 500 (about 23 s; cut the recording)\n", path.c_str(), (long long)cnt, rate,
                  clip_codes(cnt, rate));
          return 1;
        }
        sc_names.push_back(path); sc_ns.push_back(cnt); sc_rates.push_back(rate);
      }
      if (sc_names.empty()) { fprintf(stderr, "usage: --score-audio: no clip given\n"); return 1; }
    } else {
      std::ifstream f(scoreCodes);
      if (!f) { fprintf(stderr, "usage: --score-codes %s: cannot be opened\n", scoreCodes.c_str()); return 1; }
      std::string line;
      for (int ln = 1; std::getline(f, line); ln++) {
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        std::vector<int32_t> row;
        const char *p = line.c_str();
        for (;;) {
          char *end = nullptr;
          const long v = std::strtol(p, &end, 10);
          if (end == p) break;
          if (v < 0 || v >= 8192) { fprintf(stderr, "usage: --score-codes %s:%d: code %ld (0 .. 8191)\n", scoreCodes.c_str(), ln, v); return 1; }
          row.push_back((int32_t)v);
          p = end;
        }
        if (std::string(p).find_first_not_of(" \t\r") != std::string::npos || row.empty() || row.size() > 500) {
          fprintf(stderr, "usage: --score-codes %s:%d: a line holds 1 .. 500 space-separated codes\n", scoreCodes.c_str(), ln);
          return 1;
        }
        sc_n.push_back((int32_t)row.size());
        row.resize(500, 0);
        sc_codes.insert(sc_codes.end(), row.begin(), row.end());
        sc_names.push_back(scoreCodes + ":" + std::to_string(ln));
      }
      if (sc_names.empty()) { fprintf(stderr, "usage: --score-codes %s: no codes\n", scoreCodes.c_str()); return 1; }
    }
    if (sc_names.size() > 64) { fprintf(stderr, "usage: --score-audio / --score-codes: %d clips, at most 64 in one call\n", (int)sc_names.size()); return 1; }
  }
  // --aligner with a bracketed message: the brackets leave the prompt, the text they hold leaves the audio
  const bool redact = !alignerPath.empty() && message.find_first_of("[]") != std::string::npos;
  const std::string promptText = message;
  if (redact) {
    if (split_ids > 0) { fprintf(stderr, "--aligner with bracketed text cannot be combined with --split-text\n"); return 1; }
    if (voicePaths.size() > 1) { fprintf(stderr, "--aligner with bracketed text cannot be combined with several voices\n"); return 1; }
    if (stream) { fprintf(stderr, "--aligner with bracketed text cannot be combined with --stream\n"); return 1; }
    if (devices > 1 || exchange == "rccl" || shard >= 0) { fprintf(stderr, "--aligner with bracketed text cannot be combined with --devices > 1 or --exchange rccl\n"); return 1; }
    if (dry) { fprintf(stderr, "--aligner runs on the device: bracketed text cannot be combined with --dry-run 1\n"); return 1; }
    std::vector<char> clean(message.size() + 1);
    std::vector<int32_t> iv(2 * (message.size() + 1));
    if (tts_host_redact_spans(message.c_str(), clean.data(), (int)clean.size(), iv.data(), (int)message.size() + 1) < 0) {
      fprintf(stderr, "--aligner: unbalanced or nested brackets in the message\n");
      return 1;
    }
    message = clean.data();
  }
  if (stream) {
    const char *bad = !use_hifigan ? "--decoder diffusion" : !clvpPath.empty() ? "--clvp" : !cvvpPath.empty() ? "--cvvp" : split_ids > 0 ? "--split-text" : voicePaths.size() > 1 ? "several --voice" :
                      candidates > 1 ? "--candidates > 1" : (devices > 1 || shard >= 0) ? "--devices > 1" : nullptr;
    if (bad) { fprintf(stderr, "--stream serves one candidate of one voice through the HiFi-GAN decoder: it cannot be combined with %s\n", bad); return 1; }
    if (stream_stride < 1) { fprintf(stderr, "--stream-stride %d: at least 1\n", stream_stride); return 1; }
  }
  if (sampler != "ddpm" && sampler != "ddim" && sampler != "dpmpp2m") { fprintf(stderr, "--sampler %s: ddpm, ddim or dpmpp2m\n", sampler.c_str()); return 1; }
  if (!(ddim_eta >= 0.0 && ddim_eta <= 1.0)) { fprintf(stderr, "--ddim-eta %g: a value in 0 .. 1\n", ddim_eta); return 1; }
  if (!(cond_free_k >= 0.0) || !std::isfinite(cond_free_k)) { fprintf(stderr, "--cond-free-k %g: a finite value >= 0\n", cond_free_k); return 1; }
  if (cond_free != "0" && cond_free != "1") { fprintf(stderr, "--cond-free %s: 1 (guided) or 0 (unguided)\n", cond_free.c_str()); return 1; }
  if (!(diff_temp >= 0.0) || !std::isfinite(diff_temp) || !std::isfinite((float)diff_temp)) { fprintf(stderr, "--diffusion-temperature %g: a finite value >= 0\n", diff_temp); return 1; }
  if (!std::isfinite(ar_temp) || !((float)ar_temp > 0) || !std::isfinite((float)ar_temp)) { fprintf(stderr, "--temperature %g: a finite value > 0\n", ar_temp); return 1; }
  if (!(ar_top_k >= 1 && ar_top_k <= 8194) || ar_top_k != std::floor(ar_top_k)) { fprintf(stderr, "--top-k %g: an integer in 1 .. 8194\n", ar_top_k); return 1; }
  if (!(ar_top_p > 0 && ar_top_p <= 1) || !((float)ar_top_p > 0)) { fprintf(stderr, "--top-p %g: a value in (0, 1]\n", ar_top_p); return 1; }
  if (!std::isfinite(ar_pen) || !(ar_pen >= 1) || !std::isfinite((float)ar_pen)) { fprintf(stderr, "--repetition-penalty %g: a finite value >= 1\n", ar_pen); return 1; }
  if (ar_typ != 0 && (!(ar_typ > 0 && ar_typ < 1) || !((float)ar_typ > 0 && (float)ar_typ < 1))) { fprintf(stderr, "--typical-mass %g: 0 (off) or a value in (0, 1)\n", ar_typ); return 1; }
  if (ar_scope != "last" && ar_scope != "history") { fprintf(stderr, "--penalty-scope %s: last or history\n", ar_scope.c_str()); return 1; }
  if (split_ids != 0 && (devices > 1 || exchange == "rccl" || shard >= 0)) {
    fprintf(stderr, "--split-text cannot be combined with --devices > 1 or --exchange rccl (one process runs all chunks)\n");
    return 1;
  }
  if (split_ids < 0 || split_ids > 404) { fprintf(stderr, "--split-text %d: 0 (off) or 3 .. 404 text ids per chunk\n", split_ids); return 1; }
  // several voices (usage errors before any model is loaded / any worker is started)
  const int n_voices = std::max<int>(1, (int)voicePaths.size());
  const bool multi_voice = n_voices > 1;
  int n_clip_voices = 0;
  for (const std::string &c : voiceClips) n_clip_voices += !c.empty();
  // --voice-random: its SEED is an unsigned 64-bit integer, digits only
  std::vector<uint64_t> randSeed(voicePaths.size(), 0);
  int n_rand_voices = 0;
  for (size_t v = 0; v < voiceRandom.size(); v++) {
    if (!voiceRandom[v].empty()) { // a --voice-random occurrence
      const std::string t = voiceRandom[v].substr(1);
      char *end = nullptr;
      errno = 0;
      const unsigned long long sv = t.empty() || !isdigit((unsigned char)t[0]) ? 0 : strtoull(t.c_str(), &end, 10);
      if (t.empty() || !end || *end || errno == ERANGE) { fprintf(stderr, "--voice-random %s: SEED must be an unsigned 64-bit integer\n", t.c_str()); return 1; }
      randSeed[v] = (uint64_t)sv;
      n_rand_voices++;
    }
  }
  auto is_random = [&](int v) { return v < (int)voicePaths.size() && !voiceRandom[v].empty(); };
  auto is_made = [&](int v) { return v < (int)voicePaths.size() && (!voiceClips[v].empty() || is_random(v)); }; // a clip or a random voice: it brings its own latents
  const int n_file_voices = (int)voicePaths.size() - n_clip_voices - n_rand_voices;
  const int n_made_voices = n_clip_voices + n_rand_voices;
  if (n_rand_voices > 0) { // usage errors of --voice-random
    if (rlgModel.empty()) { fprintf(stderr, "--voice-random needs --random-voice-model <file> (tools/convert_weights.py --random-voice)\n"); return 1; }
    if (!use_hifigan && rlgDiffModel.empty()) { fprintf(stderr, "--voice-random with the diffusion decoder needs --random-diffusion-voice-model <file>\n"); return 1; }
    if (dry) { fprintf(stderr, "--voice-random runs on the device: it cannot be combined with --dry-run 1\n"); return 1; }
    if (devices > 1 || exchange == "rccl" || shard >= 0) { fprintf(stderr, "--voice-random cannot be combined with --devices > 1 or --exchange rccl\n"); return 1; }
  } else if (!rlgModel.empty() || !rlgDiffModel.empty()) {
    fprintf(stderr, "--random-voice-model and --random-diffusion-voice-model belong to --voice-random, which is absent\n");
    return 1;
  }
  if (n_made_voices == 0 && !diffLatentPaths.empty() && (int)diffLatentPaths.size() != n_voices) {
    fprintf(stderr, "%d --diffusion-latent for %d --voice: give none (every speaker uses the model's own latent) or one per voice, in the same order\n",
            (int)diffLatentPaths.size(), n_voices);
    return 1;
  }
  if (n_clip_voices > 0) { // usage errors of --voice-clips
    if (condModel.empty()) { fprintf(stderr, "--voice-clips needs --conditioning-model <file> (the voice-conditioning encoder)\n"); return 1; }
    if (!use_hifigan && dcondModel.empty()) { fprintf(stderr, "--voice-clips with the diffusion decoder needs --diffusion-conditioning-model <file>\n"); return 1; }
    if (dry) { fprintf(stderr, "--voice-clips runs on the device: it cannot be combined with --dry-run 1\n"); return 1; }
    if (devices > 1 || exchange == "rccl" || shard >= 0) { fprintf(stderr, "--voice-clips cannot be combined with --devices > 1 or --exchange rccl\n"); return 1; }
  } else if ((!saveVoice.empty() && n_rand_voices == 0) || !condModel.empty() || !dcondModel.empty() || !melNormsPath.empty()) {
    fprintf(stderr, "--save-voice, --conditioning-model, --diffusion-conditioning-model and --mel-norms belong to --voice-clips, which is absent\n");
    return 1;
  }
  if (n_made_voices > 0) { // what the clip and the random voices share
    if (!saveVoice.empty() && (int)saveVoice.size() != n_made_voices) {
      fprintf(stderr, "%d --save-voice for %d --voice-clips and --voice-random: give none or one per such voice, in the same order\n", (int)saveVoice.size(), n_made_voices);
      return 1;
    }
    if (!use_hifigan && (int)diffLatentPaths.size() != n_file_voices) {
      fprintf(stderr, "%d --diffusion-latent for %d --voice beside --voice-clips or --voice-random: such a voice brings its own diffusion latent, so every --voice needs one\n",
              (int)diffLatentPaths.size(), n_file_voices);
      return 1;
    }
  }
  // --cvvp (usage errors before any model is loaded)
  const bool have_cvvp = !cvvpPath.empty();
  if (!have_cvvp && have_cvvp_amount) { fprintf(stderr, "--cvvp-amount belongs to --cvvp, which is absent\n"); return 1; }
  if (have_cvvp) {
    if (!have_cvvp_amount) cvvp_amount = clvpPath.empty() ? 1.0 : 0.5;
    if (!(cvvp_amount >= 0.0 && cvvp_amount <= 1.0)) { fprintf(stderr, "--cvvp-amount %g: a value in 0 .. 1\n", cvvp_amount); return 1; }
    if (devices > 1 || exchange == "rccl" || shard >= 0) { fprintf(stderr, "--cvvp cannot be combined with --devices > 1 or --exchange rccl\n"); return 1; }
    if (n_file_voices + n_rand_voices > 0 || voicePaths.empty()) {
      fprintf(stderr, "--cvvp scores the candidates against the audio clips of their voice: a --voice latent file holds no audio (give every voice as --voice-clips)\n");
      return 1;
    }
    if (cvvp_amount > 0.0 && cvvp_amount < 1.0 && clvpPath.empty()) { fprintf(stderr, "--cvvp-amount %g blends CVVP with CLVP: it needs --clvp <file> (without --clvp the amount is 1)\n", cvvp_amount); return 1; }
  }
  // the side whose weight is 0 is neither loaded nor evaluated
  const bool use_cvvp = have_cvvp && cvvp_amount > 0.0, use_clvp = !clvpPath.empty() && !(have_cvvp && cvvp_amount >= 1.0);
  const bool rerank = use_clvp || use_cvvp;
  // the --diffusion-latent file of every voice ("" for a clip voice, or when none is given): the k-th occurrence belongs to the k-th --voice
  std::vector<std::string> diffLatentOf(n_voices);
  for (int v = 0, k = 0; v < (int)voicePaths.size(); v++)
    if (!is_made(v) && k < (int)diffLatentPaths.size()) diffLatentOf[v] = diffLatentPaths[k++];
  const bool rand_latents = n_rand_voices > 0 && !rlgDiffModel.empty(); // the random voices bring diffusion latents
  // the clip voices bring diffusion latents (the name covers both kinds from here on: with the diffusion decoder either kind must bring them)
  const bool clip_latents = (n_clip_voices > 0 && !dcondModel.empty()) || rand_latents;
  const bool clip_enc_latents = n_clip_voices > 0 && !dcondModel.empty();
  std::vector<int> saveIdx(n_voices, -1); // the --save-voice of every clip / random voice
  for (int v = 0, k = 0; v < (int)voicePaths.size(); v++)
    if (is_made(v)) saveIdx[v] = k++;
  if (multi_voice && (devices > 1 || exchange == "rccl" || shard >= 0)) {
    fprintf(stderr, "several --voice cannot be combined with --devices > 1 or --exchange rccl (the conditioning broadcast carries one voice; one process runs all turns)\n");
    return 1;
  }
  if (multi_voice && split_ids != 0 && split_ids < 3) { fprintf(stderr, "--split-text %d: 3 .. 404 text ids per chunk\n", split_ids); return 1; }
  if ((devices > 1 || exchange == "rccl") && shard < 0) { // parent: one worker process per GPU
    if (candidates % devices) { fprintf(stderr, "--candidates %d does not divide over --devices %d\n", candidates, devices); return 1; }
    std::vector<int> map;
    for (size_t p = 0; p < device_map.size();) {
      const size_t q = device_map.find(',', p);
      map.push_back(std::stoi(device_map.substr(p, q == std::string::npos ? std::string::npos : q - p)));
      if (q == std::string::npos) break;
      p = q + 1;
    }
    // One engine process per GPU. Two on ONE device is not a deployment form: round 4 saw a kernel's packed f32 FMAs return wrong sums while another
    // process's MFMA waves shared the GPU (profiles/r4_two_process_determinism.txt). The default build KEEPS the packed f32 forms (a build without them is one make
    // variable away: `make PK=...`, profiles/r5_packed_f32_ab.txt); what protects a run is this refusal — and, with --exchange files, running the workers that share a
    // device one after the other. --allow-shared-device 1 with --exchange rccl still puts two engine processes on one GPU at once (tests on a one-GPU box only).
    bool shared = false;
    for (int r = 0; r < devices; r++)
      for (int q = 0; q < r; q++)
        if ((r < (int)map.size() ? map[r] : r) == (q < (int)map.size() ? map[q] : q)) {
          shared = true;
          if (!dry && !allow_shared) {
            fprintf(stderr, "--device-map %s: workers %d and %d would share a GPU (unsupported; --allow-shared-device 1 to run anyway)\n", device_map.c_str(), q, r);
            return 1;
          }
        }
    // --allow-shared-device with --exchange files: the workers run ONE AFTER THE OTHER, so no two engine processes are ever busy on the same GPU (an RCCL exchange
    // needs all ranks alive at once — and a distinct GPU per rank, which RCCL itself enforces)
    const bool serial = shared && !dry && exchange == "files";
    if (!have_seed) // every worker must draw from the same stream
      seed = (int)(std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count() & 0x7fffffff);
    std::string id_hex;
    if (exchange == "rccl") { // the communicator's id is created here and handed to every worker
      if (dry && !getenv("TTS_RCCL_LIB")) {
        fprintf(stderr, "--dry-run with --exchange rccl needs TTS_RCCL_LIB=<stand-in library> (tests/fake_rccl.cpp): librccl cannot take the host buffers of a dry run\n");
        return 1;
      }
      RcclApi api;
      ncclUniqueId id;
      if (!api.open()) return 1;
      const ncclResult_t rr = api.GetUniqueId(&id);
      if (rr != ncclSuccess) { fprintf(stderr, "ncclGetUniqueId: %s\n", api.GetErrorString(rr)); return 1; }
      id_hex = rccl_id_to_hex(id);
    }
    std::vector<pid_t> pids;
    for (int r = 0; r < devices; r++) {
      const pid_t pid = fork();
      if (pid < 0) { perror("fork"); return 1; }
      if (pid == 0) {
        std::vector<std::string> args(argv, argv + argc);
        const std::string extra[] = {"--shard", std::to_string(r) + "/" + std::to_string(devices), "--device",
                                     std::to_string(r < (int)map.size() ? map[r] : r), "--seed", std::to_string(seed), "--end", "-"};
        if (!id_hex.empty()) { args.push_back("--rccl-id"); args.push_back(id_hex); }
        args.insert(args.end(), std::begin(extra), std::end(extra)); // later flags override earlier ones; "--end -" keeps the last pair inside i < argc-1
        std::vector<char *> av;
        for (auto &x : args) av.push_back(&x[0]);
        av.push_back(nullptr);
        execv("/proc/self/exe", av.data());
        perror("execv");
        _exit(127);
      }
      if (serial) {
        int st = 0;
        if (waitpid(pid, &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) return 1;
      } else pids.push_back(pid);
    }
    int rc = 0;
    std::vector<pid_t> alive = pids;
    while (!alive.empty()) {
      int st = 0;
      const pid_t pid = wait(&st);
      if (pid < 0) { rc = 1; break; }
      alive.erase(std::remove(alive.begin(), alive.end(), pid), alive.end());
      if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) {
        if (rc == 0 && exchange == "rccl")  // the workers still running would wait in a collective for ever
          for (pid_t p : alive) kill(p, SIGTERM);
        rc = 1;
      }
    }
    if (rc == 0 && !clvpPath.empty() && exchange == "files") { // every worker left "<output>.shard<r>.score" = "<global candidate> <score>" and that candidate's WAV
      int best_gc = -1;
      double best_score = 0;
      std::vector<int> winners;
      for (int r = 0; r < devices; r++) {
        const std::string sp = outputPath + ".shard" + std::to_string(r) + ".score";
        std::ifstream f(sp);
        int gc; double sc;
        if (!(f >> gc >> sc)) { fprintf(stderr, "missing CLVP score of worker %d\n", r); return 1; }
        winners.push_back(gc);
        if (best_gc < 0 || sc > best_score) { best_gc = gc; best_score = sc; }
        std::remove(sp.c_str());
      }
      for (int gc : winners) {
        const std::string wp = outputPath + "." + std::to_string(gc) + ".wav";
        if (gc == best_gc) { if (std::rename(wp.c_str(), outputPath.c_str())) { perror("rename"); return 1; } }
        else std::remove(wp.c_str());
      }
      printf("clvp: candidate %d kept (score %.5f)\n", best_gc, best_score);
      std::cout << "WAV file saved successfully. :^)" << std::endl;
    }
    return rc;
  }
  const int total_candidates = candidates;
  if (shard >= 0) candidates = total_candidates / nshards;
  using clk = std::chrono::steady_clock;
  const clk::time_point t_start = clk::now();
  clk::time_point t_last = t_start;
  tts_ctx *ctx = tts_create(dry ? -1 : device); // --dry-run: a host-only context (tokenizer, RNG, sampler; every stage call would fail)
  auto mark = [&](const char *what) { // --timing 1
    if (!timing) return;
    const clk::time_point t = clk::now();
    fprintf(stderr, "[timing] %-22s %8.1f ms (at %8.1f)\n", what, std::chrono::duration<double, std::milli>(t - t_last).count(),
            std::chrono::duration<double, std::milli>(t - t_start).count());
    t_last = t;
  };
  mark("tts_create");
  if (!ctx) {
    fprintf(stderr, "tts_create(%d) failed: no HIP device (this engine has no CPU path)\n", device);
    return 1;
  }
  if (have_seed) tts_seed(ctx, (uint32_t)seed);
  for (const auto &kv : engine_options)
    if (tts_set_option(ctx, kv.first.c_str(), kv.second)) return die(ctx, "--option");
  if ((have_sampler && tts_set_option(ctx, "diff_sampler", sampler == "dpmpp2m" ? (double)TTS_SAMPLER_DPMPP_2M : sampler == "ddim" ? (double)TTS_SAMPLER_DDIM : (double)TTS_SAMPLER_DDPM)) || (have_eta && tts_set_option(ctx, "ddim_eta", ddim_eta)) ||
      (have_k && tts_set_option(ctx, "cond_free_k", cond_free_k)) || (have_cond_free && tts_set_option(ctx, "cond_free", cond_free == "1" ? 1.0 : 0.0)) ||
      (have_diff_temp && tts_set_option(ctx, "diff_temperature", diff_temp)))
    return die(ctx, "--sampler");
  if ((have_temp && tts_set_option(ctx, "ar_temperature", ar_temp)) || (have_top_k && tts_set_option(ctx, "ar_top_k", ar_top_k)) ||
      (have_top_p && tts_set_option(ctx, "ar_top_p", ar_top_p)) || (have_pen && tts_set_option(ctx, "ar_repetition_penalty", ar_pen)) ||
      (have_scope && tts_set_option(ctx, "ar_penalty_scope", ar_scope == "history" ? 1.0 : 0.0)) || (have_typ && tts_set_option(ctx, "ar_typical_mass", ar_typ)))
    return die(ctx, "--temperature / --top-k / --top-p / --repetition-penalty / --penalty-scope / --typical-mass");
  if (timing) {
    char typ[48] = ""; // (the line is what it was without the flag)
    if (have_typ) snprintf(typ, sizeof typ, ", typical-mass %g", ar_typ);
    fprintf(stderr, "[timing] ar sampler temperature %g, top-k %g, top-p %g, repetition-penalty %g, penalty-scope %s%s\n", ar_temp, ar_top_k, ar_top_p, ar_pen, ar_scope.c_str(), typ);
    if (shard >= 0) fprintf(stderr, "[timing] sampler %s, ddim-eta %g, cond-free-k %g, steps %d (worker %d/%d)\n", sampler.c_str(), ddim_eta, cond_free_k, steps, shard, nshards);
    else fprintf(stderr, "[timing] sampler %s, ddim-eta %g, cond-free-k %g, steps %d\n", sampler.c_str(), ddim_eta, cond_free_k, steps);
    if (shard >= 0) fprintf(stderr, "[timing] cond-free %s, diffusion-temperature %g (worker %d/%d)\n", cond_free.c_str(), diff_temp, shard, nshards);
    else fprintf(stderr, "[timing] cond-free %s, diffusion-temperature %g\n", cond_free.c_str(), diff_temp);
    fprintf(stderr, "[timing] decoder %s\n", decoder.c_str());
    if (!use_hifigan) fprintf(stderr, "[timing] vocoder %s\n", vocoder.c_str());
  }
  if (shard >= 0) {
    tts_set_option(ctx, "rng_shard_offset", (double)(shard * candidates));
    tts_set_option(ctx, "rng_shard_total", (double)total_candidates);
  }
  // --voice-clips: every clip voice's two latents, made on the device before any other model is loaded
  std::vector<std::vector<float>> clip1024(n_voices), clip2048(n_voices);
  std::vector<std::vector<float>> cvvp_lat(n_voices); // --cvvp: every clip voice's conditioning latents [clips][latent dim], made once
  std::vector<int> cvvp_clips(n_voices, 0);
  if (n_clip_voices > 0) {
    if (use_cvvp && tts_load_cvvp(ctx, cvvpPath.c_str())) return die(ctx, "cvvp_model_load");
    if (tts_load_voice_encoder(ctx, condModel.c_str())) return die(ctx, "--conditioning-model");
    if (clip_enc_latents && tts_load_diffusion_conditioning_encoder(ctx, dcondModel.c_str())) return die(ctx, "--diffusion-conditioning-model");
    std::vector<float> norms;
    if (!melNormsPath.empty()) {
      norms.resize(80);
      std::ifstream f(melNormsPath, std::ios::binary);
      if (!f || !f.read((char *)norms.data(), 80 * sizeof(float))) { std::cerr << "Error: Unable to read 80 floats from " << melNormsPath << std::endl; return 1; }
    }
    tts_voice_audio_opts vo;
    vo.struct_size = sizeof vo;
    tts_voice_audio_opts_init(&vo);
    vo.mel_norms80 = norms.empty() ? nullptr : norms.data();
    for (int v = 0; v < n_voices; v++) {
      if (voiceClips[v].empty()) continue;
      const int k = saveIdx[v];
      std::vector<float> samples;
      std::vector<int64_t> lens;
      std::vector<int32_t> rates;
      for (size_t p = 0; p <= voiceClips[v].size();) {
        const size_t q = std::min(voiceClips[v].find(',', p), voiceClips[v].size());
        const std::string path = voiceClips[v].substr(p, q - p);
        p = q + 1;
        if (path.empty()) continue;
        int32_t rate = 0;
        const int64_t cnt = tts_read_wav(path.c_str(), nullptr, 0, &rate);
        if (cnt < 1) { fprintf(stderr, "--voice-clips %s: %s\n", path.c_str(), cnt == TTS_ERR_IO ? "cannot open, or truncated" : cnt == 0 ? "no samples" : "not a PCM16 / PCM24 / float32 RIFF WAV file"); return 1; }
        samples.resize(samples.size() + (size_t)cnt);
        if (tts_read_wav(path.c_str(), samples.data() + samples.size() - (size_t)cnt, cnt, &rate) != cnt) { fprintf(stderr, "--voice-clips %s: read error\n", path.c_str()); return 1; }
        lens.push_back(cnt); rates.push_back(rate);
      }
      if (lens.empty()) { fprintf(stderr, "--voice-clips: an empty clip list\n"); return 1; }
      clip1024[v].resize(1024);
      if (clip_enc_latents) clip2048[v].resize(2048);
      if (tts_voice_from_audio(ctx, samples.data(), lens.data(), rates.data(), (int)lens.size(), &vo, clip1024[v].data(), clip_enc_latents ? clip2048[v].data() : nullptr))
        return die(ctx, "--voice-clips");
      if (use_cvvp) {
        cvvp_clips[v] = (int)lens.size();
        cvvp_lat[v].resize((size_t)cvvp_clips[v] * tts_cvvp_latent_dim(ctx));
        if (tts_cvvp_voice_audio(ctx, samples.data(), lens.data(), rates.data(), cvvp_clips[v], &vo, cvvp_lat[v].data())) return die(ctx, "--cvvp");
      }
      if (!saveVoice.empty()) {
        std::ofstream f1(saveVoice[k] + ".bin", std::ios::binary);
        if (!f1 || !f1.write((const char *)clip1024[v].data(), 1024 * sizeof(float))) { std::cerr << "Error: Unable to write " << saveVoice[k] << ".bin" << std::endl; return 1; }
        if (clip_enc_latents) {
          std::ofstream f2(saveVoice[k] + ".diffusion.bin", std::ios::binary);
          if (!f2 || !f2.write((const char *)clip2048[v].data(), 2048 * sizeof(float))) { std::cerr << "Error: Unable to write " << saveVoice[k] << ".diffusion.bin" << std::endl; return 1; }
        }
      }
    }
    mark("voice from clips");
  }
  // --voice-random: every random voice's two latents in ONE call, before any other model is loaded; nothing here draws from the sampler's generator
  if (n_rand_voices > 0) {
    if (tts_load_random_voice(ctx, rlgModel.c_str(), rand_latents ? rlgDiffModel.c_str() : nullptr)) return die(ctx, "--random-voice-model");
    if (tts_random_voice_dim(ctx, TTS_RANDOM_VOICE_AUTO) != 1024 || (rand_latents && tts_random_voice_dim(ctx, TTS_RANDOM_VOICE_DIFFUSION) != 2048)) {
      fprintf(stderr, "--random-voice-model / --random-diffusion-voice-model: %d and %d channels, 1024 and 2048 expected\n", tts_random_voice_dim(ctx, TTS_RANDOM_VOICE_AUTO),
              tts_random_voice_dim(ctx, TTS_RANDOM_VOICE_DIFFUSION));
      return 1;
    }
    std::vector<uint64_t> seeds;
    for (int v = 0; v < n_voices; v++)
      if (is_random(v)) seeds.push_back(randSeed[v]);
    std::vector<float> r1((size_t)n_rand_voices * 1024), r2(rand_latents ? (size_t)n_rand_voices * 2048 : 0);
    if (tts_random_voice(ctx, seeds.data(), n_rand_voices, nullptr, nullptr, r1.data(), rand_latents ? r2.data() : nullptr)) return die(ctx, "--voice-random");
    for (int v = 0, j = 0; v < n_voices; v++) {
      if (!is_random(v)) continue;
      clip1024[v].assign(r1.begin() + (size_t)j * 1024, r1.begin() + (size_t)(j + 1) * 1024);
      if (rand_latents) clip2048[v].assign(r2.begin() + (size_t)j * 2048, r2.begin() + (size_t)(j + 1) * 2048);
      if (!saveVoice.empty()) {
        const int k = saveIdx[v];
        std::ofstream f1(saveVoice[k] + ".bin", std::ios::binary);
        if (!f1 || !f1.write((const char *)clip1024[v].data(), 1024 * sizeof(float))) { std::cerr << "Error: Unable to write " << saveVoice[k] << ".bin" << std::endl; return 1; }
        if (rand_latents) {
          std::ofstream f2(saveVoice[k] + ".diffusion.bin", std::ios::binary);
          if (!f2 || !f2.write((const char *)clip2048[v].data(), 2048 * sizeof(float))) { std::cerr << "Error: Unable to write " << saveVoice[k] << ".diffusion.bin" << std::endl; return 1; }
        }
      }
      j++;
    }
    mark("random voices");
  }
  if (tts_tokenizer_load(ctx, (modelsDir + "/tokenizer.json").c_str()) < 0) return die(ctx, "tokenizer");
  std::vector<int32_t> tokens(4096);
  int n = tts_tokenize(ctx, message.c_str(), tokens.data(), (int)tokens.size());
  if (n < 0) return die(ctx, "tokenize");
  tokens.resize(n);
  // --split-text: the chunks' text ids (a message that fits one chunk keeps the path without the flag)
  std::vector<std::vector<int32_t>> chunk_tokens;
  std::vector<int32_t> chunk_voice; // several --voice: the voice of every chunk (tts_split_turns: one turn per line, "<index>|" in front names its voice)
  if (multi_voice) {
    std::vector<int32_t> starts(message.size() + 1), lens(message.size() + 1), vo(message.size() + 1);
    const int k = tts_split_turns(ctx, message.c_str(), n_voices, split_ids > 0 ? split_ids : 404, starts.data(), lens.data(), vo.data(), (int)starts.size());
    if (k < 0) return die(ctx, "split-turns");
    if (k == 0) { fprintf(stderr, "the message holds no text\n"); return 1; }
    for (int c = 0; c < k; c++) {
      std::vector<int32_t> t(4096);
      const int m = tts_tokenize(ctx, message.substr(starts[c], lens[c]).c_str(), t.data(), (int)t.size());
      if (m < 0) return die(ctx, "tokenize");
      t.resize(m);
      chunk_tokens.push_back(t);
      chunk_voice.push_back(vo[c]);
    }
  } else if (split_ids > 0) {
    std::vector<int32_t> starts(message.size() + 1), lens(message.size() + 1);
    const int k = tts_split_text(ctx, message.c_str(), split_ids, starts.data(), lens.data(), (int)starts.size());
    if (k < 0) return die(ctx, "split-text");
    for (int c = 0; k > 1 && c < k; c++) {
      std::vector<int32_t> t(4096);
      const int m = tts_tokenize(ctx, message.substr(starts[c], lens[c]).c_str(), t.data(), (int)t.size());
      if (m < 0) return die(ctx, "tokenize");
      t.resize(m);
      chunk_tokens.push_back(t);
    }
  }
  const int n_chunks = (int)chunk_tokens.size(); // 0: one prompt
  const bool chunked = n_chunks > 1 || multi_voice; // the prompt-group path (several voices: also for a single chunk)

  std::vector<float> voice(1024);
  if (voicePath.empty()) { // the last voice named is a clip voice (several voices: `voices` below is what is read)
    if (!multi_voice) voice = clip1024[0];
  } else {
    std::ifstream f(voicePath, std::ios::binary);
    if (!f) { std::cerr << "Error: Unable to open file " << voicePath << std::endl; return 1; }
    f.read((char *)voice.data(), 1024 * sizeof(float));
  }
  // several voices: the table [n_voices][1024] in the order of the --voice arguments, and the diffusion latents [n_voices][2048] if given
  std::vector<float> voices, diff_latents;
  if (multi_voice) {
    voices.resize((size_t)n_voices * 1024);
    for (int v = 0; v < n_voices; v++) {
      if (is_made(v)) { std::copy(clip1024[v].begin(), clip1024[v].end(), voices.begin() + (size_t)v * 1024); continue; }
      std::ifstream f(voicePaths[v], std::ios::binary);
      if (!f || !f.read((char *)(voices.data() + (size_t)v * 1024), 1024 * sizeof(float))) {
        std::cerr << "Error: Unable to read 1024 floats from " << voicePaths[v] << std::endl;
        return 1;
      }
    }
    if (!use_hifigan && (!diffLatentPaths.empty() || clip_latents)) diff_latents.resize((size_t)n_voices * 2048);
    for (int v = 0; v < n_voices && !diff_latents.empty(); v++) {
      if (is_made(v)) { std::copy(clip2048[v].begin(), clip2048[v].end(), diff_latents.begin() + (size_t)v * 2048); continue; }
      std::ifstream f(diffLatentOf[v], std::ios::binary);
      if (!f || !f.read((char *)(diff_latents.data() + (size_t)v * 2048), 2048 * sizeof(float))) {
        std::cerr << "Error: Unable to read 2048 floats from " << diffLatentOf[v] << std::endl;
        return 1;
      }
    }
    if (dry) { // plumbing check without a device: the chunks and their voices
      for (int c = 0; c < n_chunks; c++) printf("chunk %d: voice %d, %d text ids\n", c, chunk_voice[c], (int)chunk_tokens[c].size());
      tts_destroy(ctx);
      return 0;
    }
  }
  RcclWorld world;
  const bool use_rccl = shard >= 0 && !rccl_id.empty();
  if (use_rccl) {
    if (!world.init(rccl_id, shard, nshards, dry)) { fprintf(stderr, "rccl: %s\n", world.err.c_str()); return 1; }
    // conditioning from rank 0: number of text ids, the ids, the voice latent (what SURVEY 8e's ncclBroadcast carries)
    struct { int32_t n; int32_t ids[4096]; float voice[1024]; } cond;
    memset(&cond, 0, sizeof cond);
    if (shard == 0) { cond.n = n; memcpy(cond.ids, tokens.data(), (size_t)n * 4); memcpy(cond.voice, voice.data(), 4096); }
    if (!world.broadcast(&cond, sizeof cond, 0)) { fprintf(stderr, "rccl: %s\n", world.err.c_str()); return 1; }
    n = cond.n;
    tokens.assign(cond.ids, cond.ids + n);
    memcpy(voice.data(), cond.voice, 4096);
    if (shard == test_fail_shard) { fprintf(stderr, "worker %d: --test-fail-shard\n", shard); _exit(3); } // the others are left waiting in the final exchange
  }
  if (shard >= 0 && shard == test_slow_shard) sleep(2);
  // results of the three stages (or of their stand-in under --dry-run): B output candidates, candidate c has nsamp[c] samples in `audio`
  int B = candidates, kept_gc = -1;
  double kept_score = 0;
  std::vector<float> audio;
  std::vector<size_t> nsamp;
  std::vector<int32_t> frames;
  const int B_ar = candidates;
  // The re-rankers on the B_ar candidates of one prompt (codes [B_ar][502], rows [B_ar]) of voice v: clvp * (1 - amount) + cvvp * amount, in float. Prints the
  // scores that were evaluated under `label`; returns the arg-max (-1: a call failed) and its blended score.
  auto rank_candidates = [&](const int32_t *text_ids, int n_text, const int32_t *cand_codes, const int32_t *cand_rows, int v, const std::string &label, double *best_score) {
    std::vector<float> sc(B_ar, 0.f), sv(B_ar, 0.f), blended(B_ar);
    if (use_clvp && tts_clvp_score(ctx, text_ids, n_text, cand_codes + 1, cand_rows, B_ar, 502, sc.data())) return -1;
    if (use_cvvp && tts_cvvp_score(ctx, cvvp_lat[v].data(), cvvp_clips[v], cand_codes + 1, cand_rows, B_ar, 502, sv.data())) return -1;
    const float wa = (float)(1.0 - cvvp_amount), wb = (float)cvvp_amount;
    for (int c = 0; c < B_ar; c++) blended[c] = !use_cvvp ? sc[c] : !use_clvp ? sv[c] : sc[c] * wa + sv[c] * wb;
    int best = 0;
    for (int c = 1; c < B_ar; c++)
      if (blended[c] > blended[best]) best = c;
    if (use_clvp && (use_cvvp || label.empty())) { // CLVP alone prints what it printed: one line for the single prompt, none per chunk
      printf("%sclvp scores:", label.c_str());
      for (int c = 0; c < B_ar; c++) printf(" %.5f", sc[c]);
      printf("\n");
    }
    if (use_cvvp) {
      printf("%scvvp scores:", label.c_str());
      for (int c = 0; c < B_ar; c++) printf(" %.5f", sv[c]);
      printf("\n");
    }
    *best_score = blended[best];
    return best;
  };
  if (dry) {
    // Plumbing check without a device (tests/test_distributed_cpu.py): the host sampler on fixed synthetic logits stands in for the AR stage (so the
    // RNG stream partition of a --devices run is the real one), a candidate's "audio" is its sampled ids, its CLVP score a function of them. Exercises
    // the parent's fork / exec / --shard / --seed hand-over, the per-candidate file names, the parent's pick among the workers' winners and its exit code.
    const int nsteps_dry = fixed_codes > 0 ? fixed_codes : 8, V = TTS_VOCAB_MEL;
    std::vector<float> logits((size_t)B_ar * V);
    std::vector<int32_t> prev(B_ar, 8192), ids(B_ar);
    std::vector<std::vector<float>> seqs(B_ar);
    for (int st = 0; st < nsteps_dry; st++) {
      for (int c = 0; c < B_ar; c++)
        for (int v = 0; v < V; v++) logits[(size_t)c * V + v] = 3.0f * std::sin(0.37f * (float)v + 0.11f * (float)st); // the same for every candidate: only the draws differ
      if (tts_sample(ctx, logits.data(), prev.data(), 1, B_ar, ids.data())) return die(ctx, "sample");
      for (int c = 0; c < B_ar; c++) { seqs[c].push_back((float)ids[c]); prev[c] = ids[c]; }
    }
    int best = 0;
    std::vector<double> scores(B_ar, 0.0);
    for (int c = 0; c < B_ar; c++)
      for (float v : seqs[c]) scores[c] = std::fmod(scores[c] * 31.0 + (double)v, 1009.0);
    for (int c = 1; c < B_ar; c++)
      if (scores[c] > scores[best]) best = c;
    if (!clvpPath.empty()) {
      kept_gc = (shard >= 0 ? shard * B_ar : 0) + best; kept_score = scores[best]; B = 1;
      audio = seqs[best]; nsamp.assign(1, audio.size());
      if (shard < 0) printf("clvp: candidate %d kept (score %.5f)\n", kept_gc, kept_score);
    } else {
      for (int c = 0; c < B_ar; c++) { audio.insert(audio.end(), seqs[c].begin(), seqs[c].end()); nsamp.push_back(seqs[c].size()); }
    }
  } else {
  mark("tokenizer, voice");
  // The diffusion and vocoder models do not depend on anything the autoregressive stage produces: they are read, re-laid out and uploaded on a second thread while this
  // one loads and runs the autoregressive model (round 6; the reference loads each model in front of its stage, main.cpp:5089, 5634, 6069). Their status is looked at where
  // the reference would have loaded them, so a bad file is reported at the same point of the run with the same message.
  int rc_diff = 0, rc_voc = 0;
  std::string err_diff, err_voc;
  struct Joiner { std::thread t; ~Joiner() { if (t.joinable()) t.join(); } } bg;
  if (hifiganPath.empty()) hifiganPath = modelsDir + "/ggml-hifigan-model.bin";
  if (bigvganPath.empty()) bigvganPath = modelsDir + "/ggml-bigvgan-model.bin";
  bg.t = std::thread([&]() {
    if (use_hifigan || score) return; // --score-*: the AR model alone; hifigan: its one model (56 MB, plain synchronous uploads) is loaded in front of its stage, as the reference loads every model
    rc_diff = tts_load_diffusion(ctx, (modelsDir + "/ggml-diffusion-model.bin").c_str());
    if (rc_diff) { err_diff = tts_last_error(ctx); return; }
    rc_voc = use_bigvgan ? tts_load_bigvgan(ctx, bigvganPath.c_str()) : tts_load_vocoder(ctx, (modelsDir + "/ggml-vocoder-model.bin").c_str());
    if (rc_voc) err_voc = tts_last_error(ctx);
  });
  if (tts_load_ar(ctx, (modelsDir + "/ggml-model.bin").c_str())) return die(ctx, "autoregressive_model_load");
  mark("load autoregressive");
  if (score) { // given codes under the transcript and the voice: one tts_ar_score_codes call, nothing is synthesised
    const int nc = (int)sc_names.size();
    if (!scoreAudio.empty()) {
      std::vector<float> norms;
      if (!read_norms(melNormsPath, norms)) return 1;
      if (tts_load_dvae(ctx, dvaePath.c_str())) return die(ctx, "dvae_model_load");
      tts_voice_audio_opts vo;
      vo.struct_size = sizeof vo;
      tts_voice_audio_opts_init(&vo);
      vo.mel_norms80 = norms.empty() ? nullptr : norms.data();
      std::vector<int32_t> wide((size_t)nc * 512);
      sc_n.resize(nc);
      if (tts_dvae_codes_audio(ctx, sc_samples.data(), sc_ns.data(), sc_rates.data(), nc, &vo, wide.data(), sc_n.data(), 512, nullptr)) return die(ctx, "dvae_codes_audio");
      sc_codes.assign((size_t)nc * 500, 0);
      for (int c = 0; c < nc; c++) {
        if (sc_n[c] > 500) { fprintf(stderr, "usage: --score-audio %s: %d codes, at most 500 (cut the recording)\n", sc_names[c].c_str(), sc_n[c]); return 1; }
        std::copy(wide.begin() + (size_t)c * 512, wide.begin() + (size_t)c * 512 + sc_n[c], sc_codes.begin() + (size_t)c * 500);
      }
    }
    std::vector<float> logp((size_t)nc * 501), stop((size_t)nc * 501);
    std::vector<int32_t> greedy((size_t)nc * 501);
    const int positions = scorePositions == "decode" ? TTS_SCORE_POS_DECODE : TTS_SCORE_POS_TRAIN;
    if (tts_ar_score_codes(ctx, tokens.data(), n, voice.data(), sc_codes.data(), sc_n.data(), nc, 500, positions, logp.data(), stop.data(), greedy.data(), nullptr))
      return die(ctx, "ar_score_codes");
    mark("score");
    for (int c = 0; c < nc; c++) {
      double total = 0;
      int hits = 0;
      for (int j = 0; j <= sc_n[c]; j++) {
        total += (double)logp[(size_t)c * 501 + j];
        hits += greedy[(size_t)c * 501 + j] == (j == sc_n[c] ? 8193 : sc_codes[(size_t)c * 500 + j]);
      }
      const double nll = -total / (sc_n[c] + 1);
      printf("score: %s %d %.9g %.9g %.9g %.9g %.9g\n", sc_names[c].c_str(), sc_n[c], total, nll, std::exp(nll), (double)stop[(size_t)c * 501 + sc_n[c]],
             (double)hits / (sc_n[c] + 1));
    }
    tts_destroy(ctx);
    return 0;
  }
  const int B_all = B_ar * std::max(1, n_chunks); // --split-text: candidates of all chunks
  std::vector<int32_t> codes((size_t)B_all * 502), rows(B_all);
  std::vector<float> latents((size_t)B_all * 500 * 1024);
  const float *lat_in = latents.data();
  if (chunked) {
    // all chunks in one autoregressive pass (chunk c: candidates [c B_ar, (c + 1) B_ar)), then candidate 0 or the CLVP best of every chunk
    std::vector<int32_t> ids, n_text(n_chunks), n_cand(n_chunks, B_ar);
    for (int c = 0; c < n_chunks; c++) { ids.insert(ids.end(), chunk_tokens[c].begin(), chunk_tokens[c].end()); n_text[c] = (int)chunk_tokens[c].size(); }
    int32_t nsteps = 0;
    const unsigned ar_flags = (fixed_codes > 0 ? TTS_AR_MASK_STOP : 0) | (B_ar > 1 ? TTS_AR_RETIRE : 0);
    const int rc_ar = multi_voice // every chunk is a prompt group with its turn's voice
                          ? tts_autoregressive_multi_voice(ctx, ids.data(), n_text.data(), n_chunks, voices.data(), n_voices, chunk_voice.data(), n_cand.data(),
                                                           fixed_codes > 0 ? fixed_codes : 500, ar_flags, codes.data(), rows.data(), latents.data(), &nsteps)
                          : tts_autoregressive_multi(ctx, ids.data(), n_text.data(), n_chunks, voice.data(), n_cand.data(), fixed_codes > 0 ? fixed_codes : 500,
                                                     ar_flags, codes.data(), rows.data(), latents.data(), &nsteps);
    if (rc_ar) return die(ctx, "autoregressive");
    mark("autoregressive");
    printf("tokens sampled: %d (%d chunks)\n", nsteps, n_chunks);
    if (use_clvp && tts_load_clvp(ctx, clvpPath.c_str())) return die(ctx, "clvp_model_load");
    std::vector<size_t> lat_off(B_all + 1, 0);
    for (int b = 0; b < B_all; b++) lat_off[b + 1] = lat_off[b] + (size_t)rows[b];
    std::vector<float> kept;
    std::vector<int32_t> kept_rows(n_chunks);
    for (int c = 0; c < n_chunks; c++) {
      int best = 0;
      if (rerank) { // every chunk against its own text and its own voice's clips
        double score = 0;
        best = rank_candidates(chunk_tokens[c].data(), n_text[c], codes.data() + (size_t)c * B_ar * 502, rows.data() + (size_t)c * B_ar, multi_voice ? chunk_voice[c] : 0,
                               "chunk " + std::to_string(c) + " ", &score);
        if (best < 0) return die(ctx, use_cvvp ? "clvp / cvvp" : "clvp");
      }
      const int b = c * B_ar + best;
      kept_rows[c] = rows[b];
      kept.insert(kept.end(), latents.begin() + lat_off[b] * 1024, latents.begin() + lat_off[b + 1] * 1024);
      if (multi_voice)
        printf("chunk %d: voice %d, %d text ids, candidate %d kept, %d latent rows, %d mel frames\n", c, chunk_voice[c], n_text[c], best, rows[b],
               tts_diffusion_frames(rows[b]));
      else
        printf("chunk %d: %d text ids, candidate %d kept, %d latent rows, %d mel frames\n", c, n_text[c], best, rows[b], tts_diffusion_frames(rows[b]));
    }
    latents.swap(kept);
    rows = kept_rows;
    lat_in = latents.data();
    B = n_chunks;
  } else {
    int32_t nsteps = 0;
    // More than one candidate (in this process or across --devices shards): the throughput stop rule. The reference's "all B samples of ONE
    // step are 8193" practically never fires for B > 1 (and would need a per-step exchange between shards); every sequence is the same.
    const unsigned ar_flags = (fixed_codes > 0 ? TTS_AR_MASK_STOP : 0) | (total_candidates > 1 ? TTS_AR_RETIRE : 0);
    if (stream) { // the decoder's model first: audio leaves while the loop samples
      if (tts_load_hifigan(ctx, hifiganPath.c_str())) return die(ctx, "hifigan_model_load");
      mark("load hifigan");
      if (tts_write_wav(outputPath.c_str(), nullptr, 0, 24000)) { std::cerr << "Error opening output file." << std::endl; return 1; }
      sink.f = fopen(outputPath.c_str(), "r+b");
      if (!sink.f || fseek(sink.f, 0, SEEK_END)) { std::cerr << "Error opening output file." << std::endl; return 1; }
      sink.t_ar = clk::now();
      const int rc_s = tts_hifigan_stream(ctx, tokens.data(), n, voice.data(), fixed_codes > 0 ? fixed_codes : 500, ar_flags, stream_stride, StreamSink::on_audio,
                                          &sink, codes.data(), rows.data(), nullptr, &nsteps);
      if (!rc_s) { // the two sizes of the header: RIFF chunk at byte 4, data chunk at byte 40
        const int32_t data_size = (int32_t)(sink.samples * 4), file_size = 36 + data_size;
        if (fseek(sink.f, 4, SEEK_SET) || fwrite(&file_size, 4, 1, sink.f) != 1 || fseek(sink.f, 40, SEEK_SET) || fwrite(&data_size, 4, 1, sink.f) != 1) sink.failed = true;
      }
      if (fclose(sink.f)) sink.failed = true;
      sink.f = nullptr;
      if (rc_s) return die(ctx, "hifigan_stream");
      if (sink.failed) { std::cerr << "Error writing output file." << std::endl; return 1; }
      mark("autoregressive + hifigan (streamed)");
      if (timing)
        fprintf(stderr, "[timing] first audio           %8.1f ms after the autoregressive stage began (at %8.1f), %d callbacks, stride %d\n",
                std::chrono::duration<double, std::milli>(sink.t_first - sink.t_ar).count(), std::chrono::duration<double, std::milli>(sink.t_first - t_start).count(),
                sink.calls, stream_stride);
    } else if (revoice) { // the recording's codes in place of sampled ones: no sampling, the generator is not touched
      std::vector<float> norms;
      if (!read_norms(melNormsPath, norms)) return 1;
      if (tts_load_dvae(ctx, dvaePath.c_str())) return die(ctx, "dvae_model_load");
      tts_voice_audio_opts vo;
      vo.struct_size = sizeof vo;
      tts_voice_audio_opts_init(&vo);
      vo.mel_norms80 = norms.empty() ? nullptr : norms.data();
      std::vector<int32_t> rcodes(512);
      int32_t n_codes = 0;
      if (tts_dvae_codes_audio(ctx, rv_samples.data(), &rv_n, &rv_rate, 1, &vo, rcodes.data(), &n_codes, 512, nullptr)) return die(ctx, "dvae_codes_audio");
      if (n_codes > 500) { fprintf(stderr, "usage: --revoice %s: %d codes, at most 500 (cut the recording)\n", revoicePath.c_str(), n_codes); return 1; }
      if (tts_ar_latents_for_codes(ctx, tokens.data(), n, voice.data(), rcodes.data(), n_codes, rows.data(), latents.data())) return die(ctx, "ar_latents_for_codes");
      mark("dvae codes + latents");
      printf("revoice: %d codes, %d latent rows\n", n_codes, rows[0]);
    } else {
      if (tts_autoregressive(ctx, tokens.data(), n, voice.data(), B_ar, fixed_codes > 0 ? fixed_codes : 500, ar_flags,
                             codes.data(), rows.data(), latents.data(), &nsteps))
        return die(ctx, "autoregressive");
      mark("autoregressive");
    }
    if (!revoice) printf("tokens sampled: %d\n", nsteps);
    if (fixed_codes <= 0 && !revoice) {
      std::vector<int32_t> stopped(B_ar);
      if (tts_ar_stop_status(ctx, stopped.data(), B_ar) == 0)
        for (int c = 0; c < B_ar; c++)
          if (!stopped[c]) fprintf(stderr, "warning: candidate %d sampled no stop token within 500 codes (sequence cut)\n", (shard >= 0 ? shard * B_ar : 0) + c);
    }

    // CLVP re-ranking (extension): keep the candidate whose codes (the rows the diffusion stage would consume) score best against the text
    B = B_ar;
    if (rerank) {
      if (use_clvp && tts_load_clvp(ctx, clvpPath.c_str())) return die(ctx, "clvp_model_load");
      const int best = rank_candidates(tokens.data(), n, codes.data(), rows.data(), 0, "", &kept_score);
      if (best < 0) return die(ctx, use_cvvp ? "clvp / cvvp" : "clvp");
      size_t off_rows = 0;
      for (int c = 0; c < best; c++) off_rows += (size_t)rows[c];
      lat_in = latents.data() + off_rows * 1024;
      rows[0] = rows[best];
      B = 1;
      kept_gc = (shard >= 0 ? shard * B_ar : 0) + best;
      if (total_candidates > 1) { // device noise stays keyed by the kept candidate's global id
        tts_set_option(ctx, "rng_shard_offset", (double)kept_gc);
        tts_set_option(ctx, "rng_shard_total", (double)total_candidates);
      }
      if (use_cvvp) printf("rerank: candidate %d kept (score %.5f, cvvp amount %g)\n", kept_gc, kept_score, cvvp_amount);
      else if (shard < 0) printf("clvp: candidate %d kept (score %.5f)\n", kept_gc, kept_score);
    }
  }

  bg.t.join();
  if (rc_diff) { fprintf(stderr, "diffusion_model_load: %s\n", err_diff.c_str()); return 1; }
  if (stream) { // written already
  } else if (use_hifigan) { // the kept candidates and their voices through one call
    if (tts_load_hifigan(ctx, hifiganPath.c_str())) return die(ctx, "hifigan_model_load");
    mark("load hifigan");
    size_t total = 0;
    for (int c = 0; c < B; c++) { nsamp.push_back((size_t)tts_hifigan_samples(rows[c])); total += nsamp.back(); }
    audio.assign(total, 0.f);
    if (multi_voice ? tts_hifigan_decode(ctx, lat_in, rows.data(), B, voices.data(), n_voices, chunk_voice.data(), audio.data())
                    : tts_hifigan_decode(ctx, lat_in, rows.data(), B, voice.data(), 1, nullptr, audio.data()))
      return die(ctx, "hifigan");
    mark("hifigan");
  } else {
  mark("wait for the diffusion + vocoder loads");
  if (!multi_voice && clip_latents) { // the one voice is a clip voice: its own diffusion latent
    if (tts_set_diffusion_conditioning_latent(ctx, clip2048[0].data())) return die(ctx, "diffusion_conditioning_latent");
  } else if (!diffLatentPath.empty() && !multi_voice) {
    std::vector<float> dl(2048);
    std::ifstream f(diffLatentPath, std::ios::binary);
    if (!f || !f.read((char *)dl.data(), 2048 * sizeof(float))) { std::cerr << "Error: Unable to read 2048 floats from " << diffLatentPath << std::endl; return 1; }
    if (tts_set_diffusion_conditioning_latent(ctx, dl.data())) return die(ctx, "diffusion_conditioning_latent");
  }
  size_t mel_total = 0, audio_total = 0;
  frames.assign(B, 0);
  for (int c = 0; c < B; c++) {
    frames[c] = tts_diffusion_frames(rows[c]);
    mel_total += (size_t)100 * frames[c];
    audio_total += (size_t)(use_bigvgan ? tts_bigvgan_samples(frames[c]) : tts_vocoder_samples(frames[c]));
  }
  std::vector<float> mel(mel_total);
  audio.assign(audio_total, 0.f);
  // B == 1: the reference's exact RNG order (AR uniforms, x_T, per-step noise, vocoder noise)
  const int noise_mode = (total_candidates == 1) ? TTS_NOISE_REFERENCE : TTS_NOISE_DEVICE;
  // several voices with their own diffusion latents: kept candidate c is chunk c, conditioned on its turn's voice (without: the model's own latent for all)
  if (multi_voice && !diff_latents.empty()
          ? tts_diffusion_multi_voice(ctx, lat_in, rows.data(), B, diff_latents.data(), n_voices, chunk_voice.data(), steps, nullptr, noise_mode, mel.data())
          : tts_diffusion(ctx, lat_in, rows.data(), B, steps, nullptr, noise_mode, mel.data()))
    return die(ctx, "diffusion");
  mark("diffusion");
  if (tts_diffusion_time_mlp_retries(ctx) > 0) // only ever seen while another process shares the GPU (include/tortoise_mi355x.h)
    fprintf(stderr, "[tortoise] the timestep MLP was re-evaluated %d times before two evaluations agreed\n", tts_diffusion_time_mlp_retries(ctx));
  if (rc_voc) { fprintf(stderr, "%s: %s\n", use_bigvgan ? "bigvgan_model_load" : "vocoder_model_load", err_voc.c_str()); return 1; }
  if (use_bigvgan) { // no noise: nothing is drawn from the generator
    if (tts_bigvgan(ctx, mel.data(), frames.data(), B, audio.data())) return die(ctx, "bigvgan");
  } else if (tts_vocoder(ctx, mel.data(), frames.data(), B, nullptr, noise_mode, audio.data())) return die(ctx, "vocoder");
  mark(use_bigvgan ? "bigvgan" : "vocoder");
  for (int c = 0; c < B; c++) nsamp.push_back((size_t)(use_bigvgan ? tts_bigvgan_samples(frames[c]) : tts_vocoder_samples(frames[c])));
  } // diffusion decoder
  } // !dry
  std::vector<float> redacted;
  auto write_one = [&](const float *samples, int64_t ns, int gc, bool is_output) -> bool {
    const std::string path = is_output ? outputPath : outputPath + "." + std::to_string(gc) + ".wav";
    if (redact && is_output) { // the chosen candidate without the audio of the bracketed text; a failed alignment writes nothing
      if (tts_load_aligner(ctx, alignerPath.c_str())) { die(ctx, "aligner_model_load"); return false; }
      redacted.resize((size_t)std::max<int64_t>(ns, 1));
      const int64_t kept = tts_redact_audio(ctx, samples, ns, 24000, promptText.c_str(), redacted.data(), ns);
      if (kept < 0) { die(ctx, "redact_audio"); return false; }
      fprintf(stderr, "aligner: %lld of %lld samples kept\n", (long long)kept, (long long)ns);
      samples = redacted.data(); ns = kept;
    }
    if (tts_write_wav(path.c_str(), samples, ns, 24000)) std::cerr << "Error opening output file." << std::endl;
    else if (is_output) std::cout << "WAV file saved successfully. :^)" << std::endl;
    return true;
  };
  if (stream) std::cout << "WAV file saved successfully. :^)" << std::endl;
  else if (use_rccl) {
    auto bail = [&]() { fprintf(stderr, "rccl: %s\n", world.err.c_str()); return 1; };
    std::vector<char> g;
    if (kept_gc >= 0) { // every rank's winner: (score, global candidate, samples); the best one's audio goes to rank 0
      const double mine[3] = {kept_score, (double)kept_gc, (double)audio.size()};
      if (!world.all_gather(mine, sizeof mine, g)) return bail();
      const double *all = (const double *)g.data();
      int win = 0;
      for (int r = 1; r < nshards; r++)
        if (all[3 * r] > all[3 * win]) win = r;
      std::vector<int64_t> counts(nshards);
      for (int r = 0; r < nshards; r++) counts[r] = (int64_t)all[3 * r + 2];
      std::vector<float> got;
      if (!world.send_floats(audio.data(), counts, win, 0, got)) return bail();
      if (shard == 0) {
        printf("clvp: candidate %d kept (score %.5f)\n", (int)all[3 * win + 1], all[3 * win]);
        write_one(got.data(), (int64_t)got.size(), (int)all[3 * win + 1], true);
      }
    } else { // all candidates of all ranks: rank 0 writes <output> (candidate 0) and <output>.<c>.wav
      // sizes first: every rank's per-candidate sample counts (the stages' own numbers, so a --dry-run stand-in pairs exactly like a real run)
      std::vector<int64_t> mine_ns(nsamp.begin(), nsamp.end());
      if (!world.all_gather(mine_ns.data(), (size_t)B * 8, g)) return bail();
      const int64_t *alln = (const int64_t *)g.data();
      std::vector<int64_t> counts(nshards, 0);
      for (int r = 0; r < nshards; r++)
        for (int c = 0; c < B; c++) counts[r] += alln[r * B + c];
      for (int r = 0; r < nshards; r++) {
        std::vector<float> got;
        if (!world.send_floats(audio.data(), counts, r, 0, got)) return bail();
        if (shard == 0) {
          size_t off = 0;
          for (int c = 0; c < B; c++) {
            const int64_t ns = alln[r * B + c];
            write_one(got.data() + off, ns, r * B + c, r * B + c == 0);
            off += (size_t)ns;
          }
        }
      }
    }
  } else if (chunked) { // --split-text / several voices: the chunks' audio one after the other, one file
    write_one(audio.data(), (int64_t)audio.size(), 0, true);
  } else {
    size_t off = 0;
    for (int c = 0; c < B; c++) {
      size_t ns = nsamp[c];
      const int gc = kept_gc >= 0 ? kept_gc : (shard >= 0 ? shard * B_ar : 0) + c; // global candidate index
      // the re-ranked winner of a single process IS the output; a worker's winner waits for the parent's pick under its candidate name
      if (!write_one(audio.data() + off, (int64_t)ns, gc, kept_gc >= 0 ? shard < 0 : gc == 0)) return 1;
      off += ns;
    }
    if (kept_gc >= 0 && shard >= 0) {
      std::ofstream f(outputPath + ".shard" + std::to_string(shard) + ".score");
      f << kept_gc << " " << std::setprecision(17) << kept_score << "\n";
    }
  }
  mark("write");
  if (!classifierPath.empty()) { // the score of the WAV this run wrote
    if (tts_load_classifier(ctx, classifierPath.c_str())) return die(ctx, "classifier_model_load");
    std::vector<std::string> paths;
    std::vector<float> prob;
    if (classify_wavs(ctx, outputPath, paths, prob)) return 1;
    fprintf(stderr, "classifier: %s %.9g\n", paths[0].c_str(), (double)prob[0]);
    mark("classifier");
  }
  tts_destroy(ctx);
  mark("tts_destroy");
  return 0;
}
