'use strict';
/* Node-side checks of svd_decomp(A, {algo: 'dc'}) through the JS host and the N-API addon. Driven by tests/test_node_svd_dc.py.
 *   node node_svd_dc_checks.js cpu                 (no GPU: the option is validated before any device work)
 *   node node_svd_dc_checks.js gpu <cases.json>    (GPU: host and device arrays against the oracle's singular values and the
 *                                                   reference's acceptance bounds; a call without the option is unchanged)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const EPS = 2 ** -52;
const sameBits = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;

// the bounds of tests/svd_dc_common.py: sv within 1e-12 sigma_max, descending and >= 0, check_properties with slack 1
function check(name, shape, A, ref, U, sv, V) {
  const nd_ = shape.length, M = shape[nd_ - 2], N = shape[nd_ - 1], L = Math.min(M, N);
  let batch = 1; for (let i = 0; i < nd_ - 2; i++) batch *= shape[i];
  assert.deepStrictEqual(Array.from(U.shape), [...shape.slice(0, nd_ - 2), M, L], name);
  assert.deepStrictEqual(Array.from(sv.shape), [...shape.slice(0, nd_ - 2), L], name);
  assert.deepStrictEqual(Array.from(V.shape), [...shape.slice(0, nd_ - 2), L, N], name);
  const smax = Math.max(ref.reduce((m, x) => Math.max(m, x), 0), 1e-300);
  for (let i = 0; i < ref.length; i++) assert(Math.abs(sv.data[i] - ref[i]) <= 1e-12 * smax, `${name} sv[${i}]`);
  for (let b = 0; b < batch; b++) {
    const u = U.data.subarray(b * M * L, (b + 1) * M * L), s = sv.data.subarray(b * L, (b + 1) * L), v = V.data.subarray(b * L * N, (b + 1) * L * N);
    const a = A.subarray(b * M * N, (b + 1) * M * N);
    for (let k = 0; k < L; k++) assert(s[k] >= 0 && (k === 0 || s[k] <= s[k - 1]), `${name} order`);
    let err = 0, nrm = 0;
    for (let i = 0; i < M; i++) for (let j = 0; j < N; j++) {
      let x = 0; for (let k = 0; k < L; k++) x += u[i * L + k] * s[k] * v[k * N + j];
      err += (x - a[i * N + j]) ** 2; nrm += a[i * N + j] ** 2;
    }
    assert(Math.sqrt(err) <= 48 * EPS * Math.max(M, N) * Math.max(Math.sqrt(nrm), 1e-300), `${name} reconstruction`);
    for (let p = 0; p < L; p++) for (let q = 0; q < L; q++) {
      let x = 0, y = 0;
      for (let i = 0; i < M; i++) x += u[i * L + p] * u[i * L + q];
      for (let j = 0; j < N; j++) y += v[p * N + j] * v[q * N + j];
      assert(Math.abs(x - (p === q)) <= 4 * EPS * M && Math.abs(y - (p === q)) <= 4 * EPS * N, `${name} orthogonality`);
    }
  }
}

if (mode === 'cpu') {
  const A = new la.NDArray(Int32Array.of(2, 2), Float64Array.of(1, 2, 3, 4));
  assert.throws(() => la.svd_decomp(A, {algo: 'qr'}), /^Error: svd_decomp\(A, \{algo\}\): algo must be 'jacobi' or 'dc'\.$/);
  assert.throws(() => la.svd_decomp(A, {algo: 7}), /algo must be 'jacobi' or 'dc'/);
  assert.throws(() => la.svd_dc(A, {algo: 'qr'}), /algo must be 'jacobi' or 'dc'/);      // svd_dc is svd_decomp, option included
  console.log('node svd_dc cpu checks ok');
} else if (mode === 'gpu') {
  const cases = JSON.parse(fs.readFileSync(process.argv[3]));
  let n = 0;
  for (const [name, c] of Object.entries(cases)) {
    const data = Float64Array.from(c.A), A = new la.NDArray(Int32Array.from(c.shape), data);
    const [U, sv, V] = la.svd_decomp(A, {algo: 'dc'});
    check(name, c.shape, data, c.sv, U, sv, V);
    const [Ud, svd, Vd] = la.svd_decomp(la.to_device(A), {algo: 'dc'});
    assert(Ud instanceof la.DeviceNDArray && svd instanceof la.DeviceNDArray && Vd instanceof la.DeviceNDArray, name + ' device');
    check(name + ' device', c.shape, data, c.sv, Ud, svd, Vd);
    // without the option, with an empty one and with 'jacobi' nothing changes: today's path, bit for bit
    const base = la.svd_decomp(A);
    for (const opts of [{}, {algo: 'jacobi'}, {algo: undefined}]) {
      const got = la.svd_decomp(A, opts);
      for (let k = 0; k < 3; k++) assert(sameBits(got[k].data, base[k].data), `${name} default route ${JSON.stringify(opts)}`);
    }
    n++;
  }
  console.log('node svd_dc gpu checks ok', n);
} else throw new Error('mode');
