#!/usr/bin/env node
/* Golden vectors for eigen_sym / eigenvals_sym from the real reference bundle. The reference has no symmetric solver (it plans
 * one, src/la/eigen.js:28-30), so what is recorded per case is its own nd.la.eigen(S) (src/la/eigen.js:33-80) on the symmetric
 * input: the eigenvalues as it returns them (complex128, its order) as Lam, their largest |imaginary part| (ref_max_imag),
 * ||S||_F (fro) and the seconds the call took. Where the reference throws, or returns an imaginary part above 1e-12 ||S||_F (a
 * cluster it resolves as a complex pair), Lam is not kept and the manifest says why (lam_kept: false, reason).
 * Inputs: 'uniform' cases are the lower triangle of the repo's counter-based generator nd4_uniform(seed, idx) (twin of
 * nd4js_amd/rng.py), mirrored, and are not stored; every other input is stored as S. Only numbers are written: .npy files plus
 * eigsym_manifest.json (with the sha256 of every file) under tests/golden/eigsym/.
 *
 *   ND4_REFERENCE=<path to dist/nd.js> node tools/gen_golden_eigsym.js
 *
 * Without ND4_REFERENCE the bundle is found through BASELINE.json's reference_path, as the node tests do.
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const ROOT = path.join(__dirname, '..');
function referenceBundle() {
  if (process.env.ND4_REFERENCE) return process.env.ND4_REFERENCE;
  const base = JSON.parse(fs.readFileSync(path.join(ROOT, 'BASELINE.json')));
  return path.join(base.reference_path, 'dist', 'nd.js');
}
const nd = require(referenceBundle());
const OUT = path.join(ROOT, 'tests', 'golden', 'eigsym');
fs.mkdirSync(OUT, {recursive: true});

/* ---------- the repo's counter-based generator (nd4js_amd/rng.py) ---------- */
function fmix32(h) {
  h ^= h >>> 16; h = Math.imul(h, 0x85ebca6b);
  h ^= h >>> 13; h = Math.imul(h, 0xc2b2ae35);
  h ^= h >>> 16; return h >>> 0;
}
function nd4_uniform(seed, idx) {
  const hi = fmix32((idx ^ fmix32(seed >>> 0)) >>> 0);
  const lo = fmix32((hi + 0x9E3779B9 + idx) >>> 0);
  const m = (hi >>> 5) * 67108864 + (lo >>> 6);
  return m * 2.220446049250313e-16 - 1.0;
}
function fill(seed, n) { const a = new Float64Array(n); for (let i = 0; i < n; i++) a[i] = nd4_uniform(seed, i); return a; }

/* ---------- npy + manifest ---------- */
function npy(name, typed, shape, complex) {
  let hdr = `{'descr': '${complex ? '<c16' : '<f8'}', 'fortran_order': False, 'shape': (${shape.join(', ')}${shape.length === 1 ? ',' : ''}), }`;
  const pad = 64 - ((10 + hdr.length + 1) % 64);
  hdr += ' '.repeat(pad % 64) + '\n';
  const head = Buffer.alloc(10);
  head.write('\x93NUMPY', 0, 'latin1'); head[6] = 1; head[7] = 0; head.writeUInt16LE(hdr.length, 8);
  const buf = Buffer.concat([head, Buffer.from(hdr, 'latin1'), Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength)]);
  if (buf.length > (1 << 20)) throw new Error(name + ': larger than 1 MiB');
  fs.writeFileSync(path.join(OUT, name + '.npy'), buf);
  return crypto.createHash('sha256').update(buf).digest('hex');
}
const manifest = {rng: 'fmix32-v1', comment: 'eigenvalues of the reference\'s nd.la.eigen on symmetric inputs', cases: {}};

/* ---------- inputs ---------- */
function symmetric(seed, N) { const g = fill(seed, N * N), a = new Float64Array(N * N); for (let i = 0; i < N; i++) for (let j = 0; j <= i; j++) a[N * i + j] = a[N * j + i] = g[N * i + j]; return a; }
function tridiag(N, d, e) { const a = new Float64Array(N * N); for (let i = 0; i < N; i++) { a[N * i + i] = d[i]; if (i + 1 < N) a[N * i + i + 1] = a[N * (i + 1) + i] = e[i]; } return a; }
function mirror(N, a) { for (let i = 0; i < N; i++) for (let j = 0; j < i; j++) a[N * j + i] = a[N * i + j]; return a; }
function spectrum(seed, lam) {                  // Q diag(lam) Q^T with the reflector Q = I - 2 v v^T / v^T v of a seeded v
  const N = lam.length, v = fill(seed, N), q = new Float64Array(N * N), a = new Float64Array(N * N);
  let vv = 0; for (const x of v) vv += x * x;
  for (let i = 0; i < N; i++) for (let j = 0; j < N; j++) q[N * i + j] = (i === j ? 1 : 0) - 2 * v[i] * v[j] / vv;
  for (let i = 0; i < N; i++) for (let j = 0; j <= i; j++) { let s = 0; for (let k = 0; k < N; k++) s += q[N * i + k] * lam[k] * q[N * j + k]; a[N * i + j] = s; }
  return mirror(N, a);
}
function gram(seed, N, K, sign, shift) {       // sign X X^T + shift I, X = N x K seeded
  const x = fill(seed, N * K), a = new Float64Array(N * N);
  for (let i = 0; i < N; i++) for (let j = 0; j <= i; j++) { let s = 0; for (let k = 0; k < K; k++) s += x[K * i + k] * x[K * j + k]; a[N * i + j] = sign * s + (i === j ? shift : 0); }
  return mirror(N, a);
}

/* ---------- one case ---------- */
// opts.no_reference: eigen is not called and `reason` is recorded instead (clusters_40: the reference iterates for about half an
// hour on the two 20-fold clusters and then throws 'Too many iterations for a single eigenvalue.')
function eigCase(name, family, N, S, input, opts) {
  let fro = 0; for (const x of S) fro += x * x; fro = Math.sqrt(fro);
  const m = {family, N, input, fro, files: {}, shapes: {}, sha256: {}};
  const put = (k, typed, shape, complex) => { m.sha256[k] = npy(`${name}.${k}`, typed, shape, complex); m.files[k] = `${name}.${k}.npy`; m.shapes[k] = shape; };
  if (input.kind === 'file') put('S', S, [N, N], false);
  const t0 = process.hrtime.bigint();
  if (opts && opts.no_reference) { m.lam_kept = false; m.reason = opts.no_reference; }
  else try {
    const [L] = nd.la.eigen(new nd.NDArray(Int32Array.of(N, N), Float64Array.from(S)));
    m.ref_seconds = Number(process.hrtime.bigint() - t0) / 1e9;
    const l = Float64Array.from(L.data._array);
    let im = 0; for (let i = 0; i < N; i++) im = Math.max(im, Math.abs(l[2 * i + 1]));
    m.ref_max_imag = im;
    m.lam_kept = im <= 1e-12 * fro;
    if (m.lam_kept) put('Lam', l, [N], true);
    else m.reason = 'the reference returns complex pairs for this input';
  } catch (e) {
    m.lam_kept = false; m.reason = 'the reference throws: ' + e.message;
  }
  manifest.cases[name] = m;
  console.log('wrote', name, m.lam_kept ? 'max|Im| ' + m.ref_max_imag : m.reason);
}

const DENSE_SEED = 7100;                       // tests/eigsym_common.py: dense_N is the catalogue's input of that name
for (const N of [1, 2, 3, 33, 70, 127, 128]) eigCase(`dense_${N}`, 'dense', N, symmetric(DENSE_SEED + N, N), {kind: 'uniform', seed: DENSE_SEED + N});
{ const N = 64; eigCase('zdiag_tri_64', 'zero diagonal', N, tridiag(N, new Float64Array(N), fill(8321, N - 1)), {kind: 'file'}); }
eigCase('clusters_40', 'two clusters', 40, spectrum(8330, Float64Array.from({length: 40}, (_, i) => i < 20 ? 1 : 2)), {kind: 'file'},
        {no_reference: 'the reference throws: Too many iterations for a single eigenvalue.'});
eigCase('rank5_50', 'rank 5', 50, gram(8340, 50, 5, 1, 0), {kind: 'file'});
eigCase('negdef_33', 'negative definite', 33, gram(8350, 33, 33, -1, -33), {kind: 'file'});
eigCase('identity_8', 'identity', 8, tridiag(8, new Float64Array(8).fill(1), new Float64Array(7)), {kind: 'file'});
eigCase('zero_8', 'zero', 8, new Float64Array(64), {kind: 'file'});
{ const N = 40, e = fill(8360, N - 1); for (const i of [3, 4, 20, 38]) e[i] = 0; eigCase('tri_zeros_40', 'tridiagonal with zeros in e', N, tridiag(N, fill(8361, N), e), {kind: 'file'}); }
eigCase('graded_60', 'graded', 60, spectrum(8370, Float64Array.from({length: 60}, (_, i) => Math.pow(10, -i / 10))), {kind: 'file'});

fs.writeFileSync(path.join(OUT, 'eigsym_manifest.json'), JSON.stringify(manifest, null, 1) + '\n');
