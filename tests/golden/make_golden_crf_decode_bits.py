"""Generate tests/golden/crf_decode_bits.npz: the bits that the wave kernels of the CRF head (csrc/crf.hip) and the field decoding
kernels (csrc/decode.hip) leave, recorded on the GPU.

    python tests/golden/make_golden_crf_decode_bits.py [output file]

Needs a real MI355X and the built library.  Every call goes through the public wrappers of vbg.ops (crf_posterior, crf_viterbi,
crf_path_logp, crf_nll_stable, crf_nll_stable_bwd, field_decode, field_decode_tags, field_runs, field_runs_tags), so the script runs
unchanged on any commit that has them: the committed fixture was written by the commit BEFORE the two files stated their shared steps
once, and tests/test_gpu_crf_decode_bits.py replays `crf_case` and `decode_case` below against it.

The fixture is plain data.  It holds its own inputs as bit patterns (`in:*`; a replay reads them from the file, never from a random
generator): a few base arrays, from which every case takes slices by exact operations only.  Per case and output it holds a SHA-256 of
the bytes and the words themselves where there are at most WHOLE of them, NSAMPLE words at fixed flat indices otherwise -- a mismatch
says roughly where.  Rows that belong to no document are not recorded: nothing writes them.

CASES: the smallest at which a piece shared between two kernels can go wrong.
  CRF "edge"   every template instance of the two wave kernels and both sides of every dispatch threshold, documents of 0, 1, 2, 5 rows;
  CRF "tile"   documents of 0 .. 193 rows behind three rows of no document: the 64-row tile boundaries, crf_path_logp_kernel's second
               tag prefetch, a document that starts mid-buffer;
  CRF "shift"  129 rows of emissions shifted by +50: the re-centring;
  decode       the four entries at 5 and 64 classes over row ranges that meet a wave's end, a chunk's end (255, 256, 257, 513 rows), an
               empty document and the second launch of a batch (513 documents), without and with a threshold that some scores fall
               below; the tag instances with begin tags on rows 64, 255 and 256 of a document, inside a run of that tag."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

WHOLE = 256          # outputs of at most this many 32-bit words are stored whole
NSAMPLE = 16

CRF_EDGE_NTAG = (3, 8, 9, 16, 17, 25, 32, 33, 40, 48, 49, 64)
CRF_EDGE_LENS = (0, 1, 2, 5)
CRF_TILE_NTAG = (7, 25, 64)
CRF_TILE_LENS = (0, 1, 2, 63, 64, 65, 129, 193)
CRF_TILE_LEAD = 3                                   # rows of no document in front of the first one
CRF_SHIFT_NTAG, CRF_SHIFT_LENS, CRF_SHIFT = 25, (129,), 50.0
CRF_STABLE_NTAG = (3, 33, 64)
CRF_ROWS = CRF_TILE_LEAD + sum(CRF_TILE_LENS)

DEC_C = (5, 64)
DEC_ROWS = {"r1": (1,), "r2": (2,), "r255_256_257": (255, 256, 257), "r513": (513,), "r0_3_0": (0, 3, 0), "d513": (1,) * 513}
DEC_ENTRIES = ("field_decode", "field_decode_tags", "field_runs", "field_runs_tags")
DEC_BEGIN_ROWS = (64, 255, 256)
DEC_MAX_ROWS = 768


def crf_case_ids():
    """[(family, ntag)]"""
    return [("edge", n) for n in CRF_EDGE_NTAG] + [("tile", n) for n in CRF_TILE_NTAG] + [("shift", CRF_SHIFT_NTAG)]


def decode_case_ids():
    """[(entry, C)]: one replay covers every row range, with and without the threshold"""
    return [(e, c) for e in DEC_ENTRIES for c in DEC_C]


def offsets(lens, lead=0):
    off = [lead]
    for n in lens:
        off.append(off[-1] + n)
    return off


def tag_table(C):
    """(ntag, tag_class, tag_begin): tag 0 "O", then B-1 I-1 B-2 I-2 ... while tags and classes last, START / STOP class 0; B- tags open
    a run.  C 5: 11 tags; C 64: 64 tags over classes 0 .. 31"""
    ntag = min(2 * (C - 1) + 3, 64)
    tc, tb = [0] * ntag, [0] * ntag
    for k in range(1, ntag - 2):
        tc[k], tb[k] = (k + 1) // 2, k % 2
    return ntag, tc, tb


# ---- inputs: made once by make_inputs(), stored in the fixture, read back by the replay ---------------------------------------------------
def make_inputs():
    """the base arrays, from one seeded generator.  Emissions and scores are multiples of 2^-4 (the fixture stays small); the
    transitions keep every bit"""
    g = torch.Generator().manual_seed(20261)
    q8 = lambda t: torch.round(t * 256) / 256
    inp = {
        "em": torch.round(torch.randn(CRF_ROWS, 64, generator=g) * 32) / 16,
        "trans": torch.randn(64, 64, generator=g) * 2,
        "rpath": torch.randint(0, 62, (CRF_ROWS,), generator=g, dtype=torch.int32),
        "gout": q8(torch.randn(len(CRF_TILE_LENS), generator=g)),
        "xs": torch.round(torch.randn(DEC_MAX_ROWS, 64, generator=g) * 16) / 16,
        "lm": -q8(torch.randn(DEC_MAX_ROWS, generator=g).abs()),
        "lc": -q8(torch.randn(DEC_MAX_ROWS, generator=g).abs()),
    }
    # a class per row in runs of 1 .. 6 rows (the scores get a bump there), and a tag per row in such runs, per table
    ln = torch.randint(1, 7, (DEC_MAX_ROWS,), generator=g)
    inp["cls_run"] = torch.repeat_interleave(torch.randint(0, 64, (DEC_MAX_ROWS,), generator=g, dtype=torch.int32), ln)[:DEC_MAX_ROWS].contiguous()
    for C in DEC_C:
        ntag, _, tb = tag_table(C)
        ln = torch.randint(1, 7, (DEC_MAX_ROWS,), generator=g)
        base = torch.repeat_interleave(torch.randint(0, ntag - 2, (DEC_MAX_ROWS,), generator=g, dtype=torch.int32), ln)[:DEC_MAX_ROWS]
        for name, lens in DEC_ROWS.items():
            off, N = offsets(lens), sum(lens)
            p = base[:N].clone()
            for d, n in enumerate(lens):                    # a begin tag on rows 64, 255, 256 of the document, the row in front holding it too
                for k, r in enumerate(DEC_BEGIN_ROWS):
                    if r < n:
                        p[off[d] + r - 1] = p[off[d] + r] = (1, 3, 3)[k]
                        assert tb[int(p[off[d] + r])] == 1
            if N > 8:                                       # tags outside the table
                p[N // 2 + 7], p[N // 3 + 5] = -1, ntag
            inp[f"path/{C}/{name}"] = p.contiguous()
        # the thresholds: near the median score of the longest case, so some scores fall below and some do not
        x = decode_scores(inp, C, DEC_MAX_ROWS).double()
        inp[f"thresh/scores/{C}"] = torch.softmax(x, 1).max(1).values.median().reshape(1)
        marg = decode_marginals(inp, ntag, DEC_MAX_ROWS).double()
        tc = torch.tensor(tag_table(C)[1])
        pc = tc[inp[f"path/{C}/r255_256_257"].clamp(0, ntag - 1).long()]
        sc = (marg * (tc[None, :] == pc[:, None])).sum(1)
        inp[f"thresh/tags/{C}"] = sc.median().reshape(1)
    return inp


def decode_scores(inp, C, N):
    """class scores [N, C]: the noise, + 3 at the row's run class"""
    x = inp["xs"][:N, :C].clone()
    r = torch.arange(N)
    x[r, (inp["cls_run"][:N] % C).long()] += 3.0
    return x.contiguous()


def decode_marginals(inp, ntag, N):
    """[N, ntag] positive values for the tag instances (the kernels only add them up): |noise| / 32"""
    return (inp["xs"][:N, :ntag].abs() * 0.03125).contiguous()


def crf_inputs(inp, family, ntag):
    """-> (em [N, ntag], trans, start, stop, doc_off list, random path [N] with tags -1, ntag and 2^30 in it, gold tags [N])"""
    lens, lead = {"edge": (CRF_EDGE_LENS, 0), "tile": (CRF_TILE_LENS, CRF_TILE_LEAD), "shift": (CRF_SHIFT_LENS, 0)}[family]
    off = offsets(lens, lead)
    N = off[-1]
    em = inp["em"][:N, :ntag].clone()
    if family == "shift":
        em += CRF_SHIFT
    start, stop = ntag - 2, ntag - 1
    trans = inp["trans"][:ntag, :ntag].clone()
    trans[start, :] = -10000
    trans[:, stop] = -10000
    gold = (inp["rpath"][:N] % max(ntag - 2, 1)).to(torch.int32)
    path = gold.clone()
    lo = off[0]
    path[lo + (N - lo) // 3] = -1
    path[lo + (N - lo) // 2] = ntag
    path[N - 1] = 1 << 30                                   # a document's last row
    return em.contiguous(), trans.contiguous(), start, stop, off, path, gold


# ---- the replays: one case on the device -> {name: tensor} ----------------------------------------------------------------------------
def crf_case(ops, inp, family, ntag, dev):
    em, trans, start, stop, off, rpath, gold = crf_inputs(inp, family, ntag)
    lo, hi = off[0], off[-1]
    emd, trd = em.to(dev), trans.to(dev)
    doc_off = torch.tensor(off, dtype=torch.int32, device=dev)
    out = {}
    path, score, logz, marg = ops.crf_posterior(emd, doc_off, trd, start, stop)
    out.update({"post/path": path[lo:hi], "post/score": score, "post/logz": logz, "post/marg": marg[lo:hi]})
    vpath, vscore = ops.crf_viterbi(emd, doc_off, trd, start, stop)
    out.update({"vit/path": vpath[lo:hi], "vit/score": vscore})
    for name, p in (("viterbi", path), ("random", rpath.to(dev))):
        lm, lc = ops.crf_path_logp(emd, doc_off, trd, start, stop, p.contiguous())
        out.update({f"logp/{name}/lm": lm[lo:hi], f"logp/{name}/lc": lc[lo:hi]})
    if ntag in CRF_STABLE_NTAG:
        gd = gold.to(dev)
        nll, lz, dem_unit, dtrans_unit = ops.crf_nll_stable(emd, gd, doc_off, trd, start, stop, True)
        out.update({"stable/nll": nll, "stable/logz": lz, "stable/dem_unit": dem_unit[lo:hi], "stable/dtrans_unit": dtrans_unit})
        nll0, lz0, none_a, none_b = ops.crf_nll_stable(emd, gd, doc_off, trd, start, stop, False)
        assert none_a is None and none_b is None
        out.update({"stable/loss_only/nll": nll0, "stable/loss_only/logz": lz0})
        dtrans = (inp["trans"][:ntag, :ntag] * 0.25).contiguous().to(dev)          # something to add to
        dem = ops.crf_nll_stable_bwd(dem_unit, dtrans_unit, doc_off, inp["gout"][:len(off) - 1].to(dev), dtrans)
        out.update({"stable/bwd/dem": dem[lo:hi], "stable/bwd/dtrans": dtrans})
    torch.cuda.synchronize()
    assert torch.equal(out["post/path"], out["vit/path"]) and torch.equal(out["post/score"].view(torch.int32), out["vit/score"].view(torch.int32))
    return out


def decode_case(ops, inp, entry, C, dev):
    ntag, tc, tb = tag_table(C)
    tags = entry.endswith("_tags")
    out = {}
    for name, lens in DEC_ROWS.items():
        off, N = offsets(lens), sum(lens)
        for th in (None, float(inp[f"thresh/{'tags' if tags else 'scores'}/{C}"][0])):
            if tags:
                marg, path = decode_marginals(inp, ntag, N).to(dev), inp[f"path/{C}/{name}"].to(dev)
                if entry == "field_decode_tags":
                    got = ops.field_decode_tags(marg, path, tc, tb, C, doc_off=off, thresh=th)
                else:
                    got = ops.field_runs_tags(marg, path, inp["lm"][:N].to(dev), inp["lc"][:N].to(dev), tc, tb, C, doc_off=off, thresh=th)
            else:
                got = getattr(ops, entry)(decode_scores(inp, C, N).to(dev), doc_off=off, thresh=th)
            key = f"{name}/{'none' if th is None else 'thresh'}"
            out.update({f"{key}/cls": got[0], f"{key}/score": got[1], f"{key}/{'runs' if 'runs' in entry else 'best'}": got[2]})
            if th is not None and name == "r255_256_257":
                below = int((got[1].double() < th).sum())
                assert 0 < below < N, (entry, C, below)     # the threshold does cut, and not everything
    torch.cuda.synchronize()
    return out


def run_all(ops, inp, dev):
    """{"crf/<family>/<ntag>:<name>" | "<entry>/<C>:<name>": tensor} for every case"""
    rec = {}
    for family, ntag in crf_case_ids():
        rec.update({f"crf/{family}/{ntag}:{k}": v for k, v in crf_case(ops, inp, family, ntag, dev).items()})
    for entry, C in decode_case_ids():
        rec.update({f"{entry}/{C}:{k}": v for k, v in decode_case(ops, inp, entry, C, dev).items()})
    return rec


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------------
def words(t):
    """the tensor's bytes as uint32 (every dtype here has 4 or 8 bytes)"""
    return np.ascontiguousarray(t.detach().contiguous().cpu().numpy()).reshape(-1).view(np.uint32)


def digest(t):
    """(sha256 hex of the bytes, number of words, the words when at most WHOLE, else NSAMPLE of them at fixed flat indices)"""
    a = words(t)
    if a.size > WHOLE:
        kept = a[(np.arange(NSAMPLE, dtype=np.int64) * 2654435761 + 12345) % a.size].copy()
    else:
        kept = a.copy()
    return hashlib.sha256(a.tobytes()).hexdigest(), int(a.size), kept


def save(out, inp, rec):
    """inputs as `in:<name>` (uint32 words) with their dtypes and shapes as JSON; outputs as names (JSON), sha [n, 32] uint8, sizes [n]
    and the kept words of all of them end to end"""
    arrays = {f"in:{k}": words(v) for k, v in inp.items()}
    meta = {k: [str(v.dtype).replace("torch.", ""), list(v.shape)] for k, v in inp.items()}
    dig = {k: digest(v) for k, v in rec.items()}
    np.savez_compressed(out, in_meta=np.array(json.dumps(meta, sort_keys=True)), names=np.array(json.dumps(list(dig))),
                        sha=np.array([list(bytes.fromhex(d[0])) for d in dig.values()], dtype=np.uint8),
                        sizes=np.array([d[1] for d in dig.values()], dtype=np.int64),
                        kept=np.concatenate([d[2] for d in dig.values()]).astype(np.uint32), **arrays)


def load(fix):
    """the inverse of save(), from the opened .npz -> (inputs {name: CPU tensor}, {output name: (sha256 hex, size, kept words)})"""
    inp = {}
    for k, (dt, shape) in json.loads(str(fix["in_meta"])).items():
        inp[k] = torch.from_numpy(fix[f"in:{k}"].view(np.int32).copy()).view(getattr(torch, dt)).reshape(shape)
    rec, at = {}, 0
    kept = fix["kept"]
    for name, sha, size in zip(json.loads(str(fix["names"])), fix["sha"], fix["sizes"]):
        n = int(size) if size <= WHOLE else NSAMPLE
        rec[name] = (bytes(sha.tolist()).hex(), int(size), kept[at:at + n])
        at += n
    assert at == kept.size
    return inp, rec


def main():
    for d in ("oracle", "vibertgrid-pytorch_amd", "tests"):
        sys.path.insert(0, os.path.join(ROOT, d))
    from vbg import ops
    dev = torch.device("cuda")
    inp = make_inputs()
    rec = run_all(ops, inp, dev)
    again = run_all(ops, inp, dev)
    for k in rec:                                                            # the same bits on a second call
        assert digest(rec[k])[0] == digest(again[k])[0], k
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "crf_decode_bits.npz")
    save(out, inp, rec)
    back_inp, back = load(np.load(out, allow_pickle=False))
    assert all(torch.equal(words_t(back_inp[k]), words_t(inp[k])) for k in inp) and sorted(back) == sorted(rec)
    print("wrote", out, os.path.getsize(out), "bytes", len(rec), "outputs of", len(crf_case_ids()) + len(decode_case_ids()), "cases")


def words_t(t):
    return torch.from_numpy(words(t).view(np.int32).copy())


if __name__ == "__main__":
    main()
