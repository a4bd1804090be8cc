'use strict';
/* Node-side checks of the column-pivoted QR family (rrqr_*, solve) through the JS host and the N-API addon.
 * Driven by tests/test_node_rrqr.py.
 *   node node_rrqr_checks.js cpu                        (no GPU: argument checks, loud failure)
 *   node node_rrqr_checks.js install <reference dist/nd.js>   (routing of the six names, minWork forwarding)
 *   node node_rrqr_checks.js gpu <golden dir>           (GPU: results against the reference's goldens; never reads the reference)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const NAMES = ['rrqr_decomp', 'rrqr_decomp_full', 'rrqr_rank', 'rrqr_lstsq', 'rrqr_solve', 'solve'];

function fmix32(h) { h ^= h >>> 16; h = Math.imul(h, 0x85ebca6b); h ^= h >>> 13; h = Math.imul(h, 0xc2b2ae35); h ^= h >>> 16; return h >>> 0; }
function uniform(seed, idx) {
  const hi = fmix32((idx ^ fmix32(seed >>> 0)) >>> 0), lo = fmix32((hi + 0x9E3779B9 + idx) >>> 0);
  return ((hi >>> 5) * 67108864 + (lo >>> 6)) * 2.220446049250313e-16 - 1.0;
}
function hashIdx(seed, i, mod) { return fmix32((fmix32(seed) + Math.imul(i, 0x9E3779B1)) >>> 0) % mod; }
function data(seed, n) { const d = new Float64Array(n); for (let i = 0; i < n; i++) d[i] = uniform(seed, i); return d; }
function input(NDA, seed, shape, fam) {          // tools/gen_golden_rrqr.js input() for the families used below
  const M = shape[shape.length - 2], N = shape[shape.length - 1], a = data(seed, shape.reduce((p, q) => p * q, 1));
  if (fam === 'rankdef') {
    const rank = Math.max(1, Math.min(M, N) >> 1);
    for (let i = rank; i < M; i++) for (let j = 0; j < N; j++) a[i * N + j] = 0.5 * a[((i - rank) % rank) * N + j] - 0.25 * a[((i + 1) % rank) * N + j];
  } else if (fam !== 'dense') throw new Error(fam);
  return new NDA(Int32Array.from(shape), a);
}
function loadNpy(file) {
  const buf = fs.readFileSync(file), hlen = buf.readUInt16LE(8), hdr = buf.toString('latin1', 10, 10 + hlen);
  const descr = /'descr': '([^']+)'/.exec(hdr)[1];
  const body = buf.slice(10 + hlen), ab = body.buffer.slice(body.byteOffset, body.byteOffset + body.byteLength);
  return descr === '<f8' ? new Float64Array(ab) : new Int32Array(ab);
}
function relerr(x, ref) { let n = 0, d = 0; for (let i = 0; i < ref.length; i++) { d += (x[i] - ref[i]) ** 2; n += ref[i] ** 2; } return Math.sqrt(d / Math.max(n, 1e-300)); }
const sameBits = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;

if (mode === 'cpu') {
  const I = new la.NDArray(Int32Array.of(3, 3), Float64Array.of(1, 0, 0, 0, 1, 0, 0, 0, 1)), P = new la.NDArray(Int32Array.of(3), Int32Array.of(0, 1, 2));
  const y = new la.NDArray(Int32Array.of(3, 1), Float64Array.of(1, 2, 3));
  for (const n of NAMES) assert.strictEqual(typeof la[n], 'function', n);
  assert.throws(() => la.rrqr_decomp([1, 2, 3]), /^Error: A must be at least 2D\.$/);
  assert.throws(() => la.rrqr_decomp_full([1, 2, 3]), /^Error: A must be at least 2D\.$/);
  assert.throws(() => la.rrqr_lstsq([I, I, P], y, P), /Either 2 \(\[Q,R,P\], y\) or 4 arguments/);
  assert.throws(() => la.rrqr_lstsq(I, I, new la.NDArray(Int32Array.of(3), Float64Array.of(0, 1, 2)), y), /P.dtype must be "int32"/);
  assert.throws(() => la.rrqr_lstsq(I, I, P, [[1], [2]]), /Q and y don't match/);
  assert.throws(() => la.rrqr_lstsq(I, I, new la.NDArray(Int32Array.of(2), Int32Array.of(0, 1)), y), /R and P don't match/);
  assert.throws(() => la.rrqr_solve([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]], I, P, [[1], [2], [3], [4]]), /Q @ R not square\./);
  const e = new la.SingularMatrixSolveError(y);
  assert.ok(e instanceof Error && e.x === y);
  if (la.device_count() === 0)
    for (const f of [() => la.rrqr_decomp(I), () => la.rrqr_decomp_full(I), () => la.rrqr_rank(I), () => la.rrqr_lstsq(I, I, P, y),
                     () => la.rrqr_solve(I, I, P, y), () => la.solve(I, y)])
      assert.throws(f, /no HIP device/);
  console.log('node rrqr cpu checks ok');
}

if (mode === 'install') {
  const nd = require(process.argv[3]);
  const host = {}; for (const n of NAMES) host[n] = nd.la[n];
  const nd2 = la.install(nd, {minWork: 1e5});
  const orig = nd2.la.__nd4hip_original__;
  for (const n of NAMES) {
    assert.strictEqual(typeof nd2.la[n], 'function', n);
    assert.notStrictEqual(nd2.la[n], host[n], n + ' is not routed');
    assert.strictEqual(orig[n], host[n], n);
  }
  // tiny float64 calls go to the host module's own functions: bit-identical to them
  const A = input(nd.NDArray, 5, [6, 6], 'dense'), W = input(nd.NDArray, 6, [5, 7], 'dense'), y = input(nd.NDArray, 7, [6, 2], 'dense');
  for (const [n, args] of [['rrqr_decomp', [A]], ['rrqr_decomp_full', [W]], ['rrqr_decomp', [W]]]) {
    const got = nd2.la[n](...args), want = host[n](...args);
    got.forEach((g, k) => assert.ok(sameBits(g.data, want[k].data), n));
  }
  const [Q, R, P] = host.rrqr_decomp(A);
  assert.ok(sameBits(nd2.la.rrqr_rank(R).data, host.rrqr_rank(R).data));
  assert.ok(sameBits(nd2.la.rrqr_lstsq(Q, R, P, y).data, host.rrqr_lstsq(Q, R, P, y).data));
  assert.ok(sameBits(nd2.la.rrqr_solve(Q, R, P, y).data, host.rrqr_solve(Q, R, P, y).data));
  assert.ok(sameBits(nd2.la.solve(A, y).data, host.solve(A, y).data));
  // a tiny singular system: the host module's own error class, from the host module's own function
  const S = input(nd.NDArray, 8, [6, 6], 'rankdef');
  assert.throws(() => nd2.la.solve(S, y), e => e instanceof nd.la.SingularMatrixSolveError && e.x instanceof nd.NDArray);
  if (la.device_count() === 0) {                    // 128^3 >= minWork: the accelerated path, which fails loudly here
    const B = input(nd.NDArray, 9, [128, 128], 'dense');
    for (const f of [() => nd2.la.solve(B, input(nd.NDArray, 10, [128, 1], 'dense')), () => nd2.la.rrqr_decomp(B), () => nd2.la.rrqr_decomp_full(B), () => nd2.la.rrqr_rank(B)])
      assert.throws(f, /no HIP device/);
  }
  console.log('node rrqr install checks ok');
}

if (mode === 'gpu') {
  const dir = path.join(process.argv[3], 'rrqr'), cases = JSON.parse(fs.readFileSync(path.join(dir, 'manifest.json'))).cases;
  const gold = (name, key) => loadNpy(path.join(dir, cases[name].files[key]));
  // a host module of our own (the reference is not read on the GPU machine): install() must throw ITS error class
  class HostError extends Error { constructor(x, ...args) { super(...args); if (!(x instanceof la.NDArray)) throw new Error('Assertion failed.'); this.x = x; } }
  const hostMod = {NDArray: la.NDArray, la: {matmul2: la.matmul2, SingularMatrixSolveError: HostError}};
  const nd = la.install(hostMod);
  for (const name of ['solve64', 'solve1024', 'solve_singular48']) {
    const m = cases[name], N = m.shape[0];
    const A = input(la.NDArray, m.seed, m.shape, m.family), y = new la.NDArray(Int32Array.of(N, m.J), data(m.y_seed, N * m.J));
    let x;
    if (m.singular) {
      assert.throws(() => nd.la.solve(A, y), e => { x = e.x; return e instanceof HostError && e.x instanceof la.NDArray; });
      assert.throws(() => la.solve(A, y), e => e instanceof la.SingularMatrixSolveError);
      // device operands: the error still carries a host NDArray
      assert.throws(() => nd.la.solve(la.to_device(A), la.to_device(y)), e => e instanceof HostError && e.x instanceof la.NDArray);
    } else {
      x = nd.la.solve(A, y);
      const xd = nd.la.solve(la.to_device(A), la.to_device(y));
      assert.ok(xd instanceof la.DeviceNDArray && sameBits(xd.data, x.data), name + ' device operands');
    }
    const e = relerr(x.data, gold(name, 'x'));
    assert.ok(e <= 1e-10, name + ' ' + e);
  }
  for (const name of ['sq32', 'tall300x128', 'wide128x300', 'large1024']) {
    const m = cases[name], A = input(la.NDArray, m.seed, m.shape, m.family);
    const [Q, R, P] = nd.la.rrqr_decomp(A);
    assert.ok(sameBits(P.data, gold(name, 'P')), name + ' P');
    if (!m.sampled) {
      assert.ok(relerr(Q.data, gold(name, 'Q')) <= 1e-12, name + ' Q');
      assert.ok(relerr(R.data, gold(name, 'R')) <= 1e-12, name + ' R');
    }
    assert.ok(sameBits(nd.la.rrqr_rank(R).data, gold(name, 'rank')), name + ' rank');
    const [Qd, Rd, Pd] = nd.la.rrqr_decomp(la.to_device(A));
    assert.ok(Qd instanceof la.DeviceNDArray && sameBits(Qd.data, Q.data) && sameBits(Rd.data, R.data) && sameBits(Pd.data, P.data), name + ' device');
  }
  { // the 2048^2 solve runs on the device after install
    const A = input(la.NDArray, 21, [2048, 2048], 'dense'), y = new la.NDArray(Int32Array.of(2048, 1), data(22, 2048));
    la.profile_enable(true);
    const x = nd.la.solve(A, y);
    const ops = la.profile_last().map(r => r.op);
    la.profile_enable(false);
    assert.ok(ops.includes('dqp3ls_batched'), JSON.stringify(ops));
    let res = 0, ny = 0;
    for (let i = 0; i < 2048; i++) { let s = 0; for (let j = 0; j < 2048; j++) s += A.data[i * 2048 + j] * x.data[j]; res += (s - y.data[i]) ** 2; ny += y.data[i] ** 2; }
    assert.ok(Math.sqrt(res / ny) <= 1e-9, 'solve 2048 residual ' + Math.sqrt(res / ny));
  }
  console.log('node rrqr gpu checks ok');
}
