"""No GPU: what tests/test_enc_kernels_gpu.py rests on. The harness is built by `make all` with the flags of csrc/extras.o and quotes the product's launch lines
verbatim; it refuses every invalid case before any device call (one test per rule); each float64 reference of tests/enc_cases.py agrees with an independent
torch.nn.functional restatement to 1e-12 (and the rotary embedding with the one the CVVP and CLVP oracles use); a NumPy float32 restatement of each kernel's
operation order stays inside the derived bound on every case of the matrix; every listed defect, applied to the reference, lies at least 10 bounds out on a case
built for it."""
import os
import re

import numpy as np
import pytest
import torch

import enc_cases as V
from enc_cases import ATTN, BIAS128, GROUPNORM, PLAIN64, ROT64, Case

F = torch.nn.functional


def _t(a):
    return torch.tensor(np.asarray(a, np.float64))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the build rule and the harness's text
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_build_rule_and_flags():
    mk = open(os.path.join(V.PKG, "Makefile")).read()
    rule = re.search(r"^libtts_enc_test\.so:(.*)\n\t(.*)$", mk, re.M)
    assert rule, "no rule for libtts_enc_test.so"
    deps, recipe = rule.group(1), rule.group(2)
    for d in ("testlib/enc_harness.hip", "csrc/extras.hip", "csrc/cvvp.hip", "csrc/host_logic.cpp", "$(HDRS)"):
        assert d in deps, d
    assert "$(CXXFLAGS) -mllvm -amdgpu-mfma-vgpr-form $(PK) -shared" in recipe  # the flags of csrc/extras.o and csrc/cvvp.o
    assert re.search(r"^csrc/diffusion\.o csrc/extras\.o csrc/cvvp\.o: CXXFLAGS \+= -mllvm -amdgpu-mfma-vgpr-form$", mk, re.M)
    assert "libtts_enc_test.so" in re.search(r"^all:(.*)$", mk, re.M).group(1)
    assert "libtts_enc_test.so" in re.search(r"^clean:\n\t(.*)$", mk, re.M).group(1)
    src = open(V.SRC).read()
    assert '#include "../csrc/extras.hip"' in src and '#include "../csrc/cvvp.hip"' in src  # the kernels as the product compiles them
    assert os.path.exists(V.LIB_PATH), "build() makes the harness"


def test_harness_restates_the_products_launch_lines():
    product = open(os.path.join(V.PKG, "csrc", "extras.hip")).read() + open(os.path.join(V.PKG, "csrc", "cvvp.hip")).read()
    src = open(V.SRC).read()
    quoted = re.findall(r"^\s*// (\w+): (.*<<<.*\);)\s*$", src, re.M)
    assert len(quoted) == 16, quoted
    for site, line in quoted:
        assert line in product, (site, line)
        assert re.search(r"\b%s\(" % site, product), site
    # every kernel the harness launches is quoted, and only the instantiations a launch site uses are instantiated
    body = src[src.index("tts_enc_test_run(const"):]
    launched = set(re.findall(r"^\s*(?:else )?(?:if \(.*?\) )?(\w+(?:<[^<>]*>)?)<<<", body, re.M))
    assert launched == {re.match(r"(?:else )?(?:if \(.*?\) )?(\w+(?:<[^<>]*>)?)<<<", l).group(1) for _, l in quoted}, launched
    assert len(launched) == 16


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# refusals: one test per validation rule, none with a device
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _with(c, **kw):
    p = dict(c.p)
    p.update(kw)
    return Case(c.op, c.family, **{k: v for k, v in p.items() if v is not None})


def _good():
    return dict(embed=V.embed_case(128), rms=V.rmsnorm_case(128), attn=V.attn_case(ROT64, [5, 3], first=1), bias=V.attn_case(BIAS128, [5], heads=2),
                pool=V.pool_case(128, [2, 1]), gn=V.gn_case(512, [3, 2]), mel=V.mel_rows_case([3, 2]), i3=V.im2col_case(3, [5, 2], 100, 320, True),
                i3r=V.im2col_case(3, [5, 2], 128, 384, False), i5=V.im2col_case(5, [5], 80, 448, True), geglu=V.geglu_case(128), rowmean=V.rowmean_case(512, [2]),
                rownorm=V.rownorm_case(128))


i32 = lambda *v: np.array(v, np.int32)
RULES = [
    ("op below the range", "rms", dict(), dict(op=-1)), ("op above the range", "rms", dict(), dict(op=11)),
    ("no input", "rms", dict(), dict(in_=None)), ("no output", "rms", dict(), dict(out=None)),
    ("no rows", "rms", dict(rows=0), {}), ("more rows than the cap", "rms", dict(rows=V.MAX_ROWS + 1), {}),
    ("no columns", "rms", dict(dim=0), {}), ("poison flag out of range", "attn", dict(poison=2), {}),
    ("no sequences", "attn", dict(nseq=0), {}), ("more sequences than the cap", "attn", dict(nseq=V.MAX_SEQ + 1), {}),
    ("embed: token below 0", "embed", dict(tok=i32(*([-1] + [0] * 20))), {}), ("embed: token past the table", "embed", dict(tok=i32(*([37] + [0] * 20))), {}),
    ("embed: no tokens", "embed", dict(tok=None), {}), ("embed: empty table", "embed", dict(vocab=0), {}), ("embed: table above the cap", "embed", dict(vocab=V.MAX_VOCAB + 1), {}),
    ("embed: dim no multiple of 128", "embed", dict(dim=100), {}),
    ("rmsnorm: no gain", "rms", dict(p0=None), {}), ("rmsnorm: dim above 1024", "rms", dict(dim=1152), {}), ("rmsnorm: dim no multiple of 128", "rms", dict(dim=192), {}),
    ("rownorm: no bias", "rownorm", dict(p1=None), {}), ("rownorm: dim above 1024", "rownorm", dict(dim=1152), {}),
    ("geglu: ff no multiple of 128", "geglu", dict(dim=100), {}), ("geglu: ff above the cap", "geglu", dict(dim=1664), {}),
    ("attn: variant out of range", "attn", dict(variant=3), {}), ("attn: inner no multiple of DH", "bias", dict(dim=192), {}),
    ("attn: inner above 2048", "attn", dict(dim=2112), {}), ("attn: a table without BIAS", "attn", dict(p0=np.zeros(384, np.float32)), {}),
    ("attn: BIAS without a table", "bias", dict(p0=None), {}), ("attn: no layout", "attn", dict(start=None), {}),
    ("attn: an empty sequence", "attn", dict(len=i32(5, 0)), {}), ("attn: sequences overlap", "attn", dict(start=i32(1, 5)), {}),
    ("attn: sequences out of order", "attn", dict(start=i32(6, 1), len=i32(3, 5)), {}), ("attn: a sequence past the last row", "attn", dict(len=i32(5, 5)), {}),
    ("attn: a negative start", "attn", dict(start=i32(-1, 6)), {}),
    ("pool: dim above 1024 (acc[4])", "pool", dict(dim=1152), {}), ("pool: no weight", "pool", dict(p0=None), {}), ("pool: a sequence past the last row", "pool", dict(len=i32(2, 3)), {}),
    ("rowmean: dim above 1024", "rowmean", dict(dim=1152), {}), ("rowmean: an empty sequence", "rowmean", dict(len=i32(0)), {}),
    ("groupnorm: a width that is not instantiated", "gn", dict(dim=768), {}), ("groupnorm: no bias", "gn", dict(p1=None), {}), ("groupnorm: clips overlap", "gn", dict(start=i32(0, 2)), {}),
    ("mel_rows: not 80 bands", "mel", dict(dim=100), {}), ("mel_rows: a negative offset", "mel", dict(mel_off=np.array([-1, 240], np.int64)), {}),
    ("mel_rows: a clip past the buffer", "mel", dict(mel_off=np.array([0, 241], np.int64)), {}), ("mel_rows: no offsets", "mel", dict(mel_off=None), dict(in_count=400)),
    ("im2col3: kpad below 3 cin", "i3", dict(kpad=256), {}), ("im2col3: kpad no multiple of 64", "i3", dict(kpad=330), {}), ("im2col3: kpad above the cap", "i3", dict(kpad=V.MAX_COLS + 64), {}),
    ("im2col3: an output length that is not the convolution's", "i3", dict(out_len=i32(2, 1)), {}), ("im2col3: output rows past the buffer", "i3", dict(out_rows=4), {}),
    ("im2col3: layout variant out of range", "i3", dict(variant=2), {}), ("im2col3: an empty clip", "i3", dict(len=i32(0, 2)), {}),
    ("im2col3 rows: input rows past the buffer", "i3r", dict(rows=7), {}), ("im2col3 rows: no input layout", "i3r", dict(start=None), {}),
    ("im2col5: kpad below 5 cin", "i5", dict(kpad=384), {}), ("im2col5: a clip past the buffer", "i5", dict(mel_off=np.array([1], np.int64)), {}),
    ("im2col5: no output layout", "i5", dict(out_start=None), {}),
]


def test_the_base_cases_are_accepted():
    for k, c in _good().items():
        assert V.validate(c) == 0, k
    for c in V.copy_cases() + V.norm_cases() + V.attn_product_cases() + [c for v in range(3) for c in V.attn_cases(v)]:
        assert V.validate(c) == 0, c.name()


@pytest.mark.parametrize("what,base,change,override", RULES, ids=[r[0] for r in RULES])
def test_refused_before_any_device_call(what, base, change, override):
    import ctypes as C
    c = _with(_good()[base], **change)
    assert V.validate(c, **override) == V.HIP_INVALID, what
    s, keep = c.struct(**override)
    assert V.lib().tts_enc_test_out_bytes(C.byref(s)) == -V.HIP_INVALID
    assert V.lib().tts_enc_test_run(C.byref(s)) == V.HIP_INVALID  # (this test runs without a device: a HIP call would answer with another status)


def test_null_case_is_refused():
    assert V.lib().tts_enc_test_run(None) == V.HIP_INVALID and V.lib().tts_enc_test_validate(None) == V.HIP_INVALID


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the references against independent restatements
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _rotate_half(t, pos):
    """x-transformers' apply_rotary_pos_emb on the first 32 dims, as oracle.Clvp.encode spells it: t cos + rotate_half(t) sin, freqs = cat(f, f)"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, 32, 2, dtype=torch.float64) / 32.0))
    fr = torch.outer(_t(pos), inv)
    fr = torch.cat([fr, fr], -1)
    tl = t[..., :32]
    rot = torch.cat([-tl[..., 16:], tl[..., :16]], -1)
    return torch.cat([tl * fr.cos() + rot * fr.sin(), t[..., 32:]], -1)


def test_rotary_is_the_oracles():
    import cvvp_ref
    rs = np.random.RandomState(0)
    t = rs.randn(2, 37, 64)
    mine = np.stack([V.rot_ref(t[h], np.arange(37.0))[0] for h in range(2)])
    assert np.abs(mine - cvvp_ref.NumpyCVVP.rotate(None, t)).max() <= 1e-12
    assert np.abs(mine - _rotate_half(_t(t), np.arange(37.0)).numpy()).max() <= 1e-12


def test_clvp_oracle_layer_is_rmsnorm_attention_layernorm():
    """oracle.Clvp.encode in float64 on a one-layer model whose projections are identities and whose feed-forward is zero: LayerNorm(x + attention(rmsnorm(x)))"""
    import oracle as O
    d, n = 64, 23
    rs = np.random.RandomState(1)
    g = 1.0 + 0.2 * rs.randn(d)
    lw, lb = 1.0 + 0.2 * rs.randn(d), 0.1 * rs.randn(d)
    a, f = "text_transformer.transformer.attn_layers.layers.0.", "text_transformer.transformer.attn_layers.layers.1."
    w = {"text_emb.weight": np.zeros(256 * d), a + "0.g": g, a + "1.to_q.weight": np.eye(d), a + "1.to_k.weight": np.eye(d), a + "1.to_v.weight": np.eye(d),
         a + "1.to_out.weight": np.eye(d), a + "1.to_out.bias": np.zeros(d), f + "0.g": np.ones(d), f + "1.net.0.proj.weight": np.zeros((2 * d, d)),
         f + "1.net.0.proj.bias": np.zeros(2 * d), f + "1.net.3.weight": np.zeros((d, d)), f + "1.net.3.bias": np.zeros(d),
         "text_transformer.transformer.norm.weight": lw, "text_transformer.transformer.norm.bias": lb}

    class Model:
        def tensor(self, name):
            return np.asarray(w[name], np.float64).reshape(-1)

    x = rs.randn(n, d)
    want = O.Clvp(Model(), np.float64).encode("text_transformer", x)
    y = V.rmsnorm_reference(Case(V.RMSNORM, x=x, rows=n, dim=d, p0=g))[0]
    c = Case(ATTN, x=np.concatenate([y, y, y], 1), variant=ROT64, rows=n, nseq=1, start=[0], len=[n], dim=d)
    o = V.attn_reference(c, 0, 0, stage=False)[0]
    got = np.concatenate([V._norm_block(r[None, :], lw, lb, 9)[0] for r in x + o])
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("variant", [ROT64, PLAIN64, BIAS128], ids=["rot64", "plain64", "bias128"])
def test_attention_reference_against_torch(variant):
    DH = V.attn_dh(variant)
    for c in (V.attn_case(variant, [130, 37], "flat", "sharp", first=3), V.attn_case(variant, [70], "dom5", "smooth")):
        x = c.x.astype(np.float64)
        for s, (r0, n) in enumerate(zip(c.start, c.len)):
            for h in range(c.heads):
                q, k, v = (_t(x[r0:r0 + n, i * c.dim + h * DH:i * c.dim + (h + 1) * DH]) for i in range(3))
                mask = None
                if variant == ROT64:
                    q, k, v = (_rotate_half(t, np.arange(float(n))) for t in (q, k, v))
                if variant == BIAS128:
                    dist = np.arange(n)[None, :] - np.arange(n)[:, None]
                    mask = _t(c.p0[h][np.where(dist > 0, 64, 0) + np.minimum(np.abs(dist), 63)])
                want = F.scaled_dot_product_attention(q[None], k[None], v[None], attn_mask=mask)[0].numpy()
                assert np.abs(V.attn_reference(c, s, h, stage=False)[0] - want).max() <= 1e-12, (c.name(), s, h)
                # the staged reference is the same attention on k and v rounded to fp16
                k16, v16 = _t(V.rn16(k.numpy())), _t(V.rn16(v.numpy()))
                want = F.scaled_dot_product_attention(q[None], k16[None], v16[None], attn_mask=mask)[0].numpy()
                assert np.abs(V.attn_reference(c, s, h)[0] - want).max() <= 1e-12, (c.name(), s, h)


def test_norm_references_against_torch():
    worst = 0.0
    for c in V.norm_cases():
        y = V.reference(c)[0]
        x = _t(c.x)
        if c.op == V.RMSNORM:
            want = F.normalize(x, dim=-1, eps=1e-8 * c.dim ** 0.5) * c.dim ** 0.5 * _t(c.p0)
        elif c.op == V.ROWNORM:
            want = F.layer_norm(x, (c.dim,), _t(c.p0), _t(c.p1), 1e-5)
        elif c.op == V.POOL:
            want = torch.stack([F.layer_norm(x[r0:r0 + n], (c.dim,), _t(c.p0), _t(c.p1), 1e-5).mean(0) for r0, n in zip(c.start, c.len)])
        elif c.op == V.ROWMEAN:
            want = torch.stack([x[r0:r0 + n].mean(0) for r0, n in zip(c.start, c.len)])
        elif c.op == V.GEGLU:
            want = x[:, :c.dim] * F.gelu(x[:, c.dim:])
        else:
            want = torch.zeros_like(x)
            for r0, n in zip(c.start, c.len):
                want[r0:r0 + n] = F.group_norm(x[r0:r0 + n].T[None], 32, _t(c.p0), _t(c.p1), 1e-5)[0].T
        want = want.numpy().reshape(-1)
        scale = max(1.0, float(np.abs(want).max()), float(np.abs(c.x).max()))  # 1e-12 of the data's magnitude: the 1e4 clips of the `neighbour` family
        worst = max(worst, float(np.abs(y - want).max() / scale))
        assert np.abs(y - want).max() <= 1e-12 * scale, c.name()
    print("norm references against torch.nn.functional: %.2e" % worst)


def test_copy_references_against_torch():
    for c in V.copy_cases():
        bits, wr = V.copy_reference(c)
        if c.op == V.EMBED:
            want = F.embedding(torch.tensor(c.tok.astype(np.int64)), torch.tensor(c.x)).numpy().view(np.uint32).reshape(-1)
            assert (bits == want).all()
            continue
        width = 128 if c.op == V.MEL_ROWS else c.kpad
        bits, wr = bits.reshape(-1, width), wr.reshape(-1, width)
        starts, lens = (c.start, c.len) if c.op == V.MEL_ROWS else (c.out_start, c.out_len)
        live = np.zeros(len(bits), bool)
        for m, r0, n in zip(c.clips, starts, lens):
            live[r0:r0 + n] = True
            m = torch.tensor(np.ascontiguousarray(m)).to(torch.float16)  # [cin][T], rounded once
            if c.op == V.MEL_ROWS:
                want = F.pad(m.T, (0, 48))
            else:  # conv1d's unfold: [cin * taps][Tout] with k = c * taps + tap -> rows [Tout][tap * cin + c], zero padded to kpad
                taps, cin = c.taps, c.dim
                u = F.unfold(m.float()[None, :, None, :], (1, taps), padding=(0, taps // 2), stride=(1, 2))[0]
                want = F.pad(u.reshape(cin, taps, -1).permute(2, 1, 0).reshape(-1, taps * cin), (0, c.kpad - taps * cin)).to(torch.float16)
            assert want.shape[0] == n, c.name()
            assert (bits[r0:r0 + n] == want.numpy().view(np.uint16)).all(), c.name()
        assert (wr == live[:, None]).all() and (bits[~live] == V.SENTINEL * 0x0101).all(), c.name()
        if c.op == V.MEL_ROWS:
            assert (bits[live][:, 80:] == 0).all()


def test_coded_inputs_are_distinct_after_the_rounding():
    v = V.coded((29000,)).astype(np.float16)
    assert len(np.unique(v.view(np.uint16))) == 29000 and np.isfinite(v.astype(np.float32)).all()
    assert (v.astype(np.float32) != V.coded((29000,))).mean() > 0.5  # the rounding is exercised


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the bounds hold for a correct kernel: the float32 restatements on the whole matrix
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _inside(cases):
    worst = {}
    for c in cases:
        y, b, wr = V.reference(c)
        e = V.emulate(c)
        assert e.shape == y.shape, c.name()
        bad, r = V.judge(e[wr], y[wr], b[wr])
        assert bad == 0, (c.name(), bad, r)
        worst[c.kernel()] = max(worst.get(c.kernel(), 0.0), r)
    print({k: round(v, 4) for k, v in worst.items()})
    return worst


def test_f32_restatements_stay_inside_the_bounds_norms():
    worst = _inside(V.norm_cases())
    assert len(worst) == 8
    for c in V.norm_cases():
        if c.op == V.RMSNORM:  # the all-zero row: exact zeros through the clamp
            assert (V.rmsnorm_emulate(c)[3] == 0).all() and (V.rmsnorm_reference(c)[0][3] == 0).all()


@pytest.mark.parametrize("variant", [ROT64, PLAIN64, BIAS128], ids=["rot64", "plain64", "bias128"])
def test_f32_restatements_stay_inside_the_bounds_attention(variant):
    _inside(V.attn_cases(variant) + [c for c in V.attn_product_cases() if c.variant == variant])


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the bounds are sharp: every listed defect lies at least 10 bounds out on a case built for it
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _out_by(ref, mutated, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(mutated - ref) / bound
    return float(np.where(np.isnan(r), np.inf, r).max())


def _two(variant, table="sharp"):  # a sequence whose neighbour's first key would dominate it
    return V.attn_case(variant, [130, 5], "dom0", table, first=3)


ATTN_DEFECTS = [
    ("last key dropped", "drop_last", (ROT64, PLAIN64, BIAS128), lambda v: V.attn_case(v, [517], "dom516", "sharp")),
    ("key n visible", "admit_n", (ROT64, PLAIN64, BIAS128), _two),
    ("the last chunk read to its full KC", "stale_chunk", (ROT64, PLAIN64, BIAS128), lambda v: V.attn_case(v, [V.attn_kc(v) + 1], "ramp_up", "sharp")),
    ("rotary pairs (d, d + 1)", "pairs_adjacent", (ROT64,), lambda v: V.attn_case(v, [130], "flat")),
    ("frequency 10000^(-d / 32)", "freq_32", (ROT64,), lambda v: V.attn_case(v, [130], "flat")),
    ("v unrotated", "v_unrotated", (ROT64,), lambda v: V.attn_case(v, [517], "dom100")),
    ("v rotated at the query's position", "v_at_query", (ROT64,), lambda v: V.attn_case(v, [517], "dom100")),
    ("positions from global rows", "global_rows", (ROT64,), lambda v: V.attn_case(v, [130], "flat", first=3, tail=2)),
    ("positions of the second z-block restart at 0", "z_restart", (ROT64, BIAS128), lambda v: V.attn_case(v, [257], "flat", "sharp")),
    ("rotary on dims 32..63 too", "rot_upper", (ROT64,), lambda v: V.attn_case(v, [130], "flat")),
    ("the scale of the other DH", "other_scale", (ROT64, PLAIN64, BIAS128), lambda v: V.attn_case(v, [130], "flat", "smooth")),
    ("bias sides swapped", "sides_swapped", (BIAS128,), lambda v: V.attn_case(v, [130], "flat", "sharp")),
    ("saturation at 62", "saturate_62", (BIAS128,), lambda v: V.attn_case(v, [130], "flat", "sharp")),
    ("saturation at 64", "saturate_64", (BIAS128,), lambda v: V.attn_case(v, [130], "flat", "sharp")),
    ("distance off by one", "distance_plus_1", (BIAS128,), lambda v: V.attn_case(v, [130], "flat", "sharp")),
    ("head h with head h + 1's table", "next_head_table", (BIAS128,), lambda v: V.attn_case(v, [130], "flat", "sharp")),
    ("head columns at stride 64 under DH 128", "head_stride_64", (BIAS128,), lambda v: V.attn_case(v, [130], "flat", "sharp")),
]
assert [d[1] for d in ATTN_DEFECTS] == V.ATTN_MUTS


@pytest.mark.parametrize("what,mut,variants,build", ATTN_DEFECTS, ids=[d[1] for d in ATTN_DEFECTS])
def test_attention_defects_fall_ten_bounds_out(what, mut, variants, build):
    for v in variants:
        c = build(v)
        for h in range(1 if mut == "head_stride_64" else 0, c.heads):  # (head 0 starts at column 0 under either stride)
            o, b = V.attn_reference(c, 0, h)
            r = _out_by(o, V.attn_reference(c, 0, h, mut=mut)[0][:len(o)], b)
            print("%s, %s, head %d: %.1f bounds" % (what, V.ATTN_NAMES[v], h, r))
            assert r >= 10, (what, v, h, r)


GN_DEFECTS = [("statistics per row", "per_row", "gauss"), ("a neighbour clip's row included", "neighbour_row", "neighbour"), ("divisor G T - 1", "unbiased", "gauss"),
              ("eps 1e-6", "eps_1e-6", "tiny"), ("the group width of another D", "other_width", "gauss")]


@pytest.mark.parametrize("what,mut,family", GN_DEFECTS, ids=[d[1] for d in GN_DEFECTS])
def test_groupnorm_defects_fall_ten_bounds_out(what, mut, family):
    for D in (512, 1024, 2048):
        # (the unbiased divisor moves the output by 1 / (2 G T): a one-row clip is where that is many fp16 steps)
        c = V.gn_case(D, [1, 2] if mut == "unbiased" else [9, 5], "neighbour" if family == "neighbour" else "gauss", first=2)
        if family == "tiny":  # a clip whose variance is of the order of eps: the only place eps matters
            c = _with(c, x=(c.x * np.float32(3e-3)))
        y, b, wr = V.gn_reference(c)
        r = _out_by(y[wr], V.gn_reference(c, mut=mut)[0][wr], b[wr])
        print("%s, D %d: %.1f bounds" % (what, D, r))
        assert r >= 10, (what, D, r)


ROW_DEFECTS = [("rmsnorm: dim^-1/2 dropped", V.rmsnorm_case, V.rmsnorm_reference, "no_dim_scale"), ("rmsnorm: mean subtracted", V.rmsnorm_case, V.rmsnorm_reference, "mean_subtracted"),
               ("rmsnorm: clamp dropped", V.rmsnorm_case, V.rmsnorm_reference, "no_clamp"), ("geglu: halves swapped", V.geglu_case, V.geglu_reference, "halves_swapped"),
               ("geglu: tanh GELU", V.geglu_case, V.geglu_reference, "tanh"), ("pool: mean before LayerNorm", lambda d: V.pool_case(d, [3, 1, 2]), V.pool_reference, "mean_first"),
               ("pool: divisor maxlen", lambda d: V.pool_case(d, [3, 1, 2]), V.pool_reference, "divisor_maxlen")]


@pytest.mark.parametrize("what,build,ref,mut", ROW_DEFECTS, ids=[d[3] for d in ROW_DEFECTS])
def test_row_kernel_defects_fall_ten_bounds_out(what, build, ref, mut):
    for d in (128, 384):
        c = build(d)
        y, b = ref(c)
        m = ref(c, mut=mut)[0]
        if mut == "no_clamp":  # NaN on the all-zero row
            assert np.isnan(m[3]).all() and not np.isnan(y).any()
            continue
        r = _out_by(y, m, b)
        print("%s, %d: %.1f bounds" % (what, d, r))
        assert r >= 10, (what, d, r)


COPY_DEFECTS = [("im2col: order c taps + tap", "channel_major_k", (V.IM2COL3, V.IM2COL5)), ("im2col: padding off by one", "pad_off_by_one", (V.IM2COL3, V.IM2COL5)),
                ("im2col: Tin taken for Tout", "tin_for_tout", (V.IM2COL3, V.IM2COL5)), ("mel_rows: the transposed index", "transposed", (V.MEL_ROWS,))]


@pytest.mark.parametrize("what,mut,ops", COPY_DEFECTS, ids=[d[1] for d in COPY_DEFECTS])
def test_copy_kernel_defects_change_bits(what, mut, ops):
    """bit for bit: any changed bit is a failure; every case with more than one input frame shows each defect"""
    seen = 0
    for c in V.copy_cases():
        if c.op not in ops or max(c.len) < 3:
            continue
        bits, wr = V.copy_reference(c)
        mb, mw = V.copy_reference(c, mut=mut)
        assert (bits != mb).any() or (wr != mw).any(), (what, c.name())
        seen += 1
    assert seen >= 3
