'use strict';
/* Node-side checks of the selected singular triplets through the JS host and the N-API addon: svd_decomp(A, {subset}), svd_vals,
 * bidiag_svd(d, e, {subset}), bidiag_svdvals. Driven by tests/test_node_svd_subset.py.
 *   node node_svd_subset_checks.js cpu                 (no GPU: the argument errors, the empty subset)
 *   node node_svd_subset_checks.js gpu <cases.json>    (GPU: host arrays and DeviceNDArrays give the bits of the Python result)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const sameBits = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const eye = N => { const d = new Float64Array(N * N); for (let i = 0; i < N; i++) d[i * N + i] = 1; return new la.NDArray(Int32Array.of(N, N), d); };
const vec = (...x) => new la.NDArray(Int32Array.of(x.length), Float64Array.from(x));
const BAD = [[3, 2], [-1, 2], [0, 5], [0], [0, 1, 2], 3, [0.5, 2], 'ab'];

function argumentErrors() {
  for (const bad of BAD) {
    assert.throws(() => la.svd_decomp(eye(4), {subset: bad}), err => /subset must be \[i0, i1\] with 0 <= i0 <= i1 <= min\(M, N\)/.test(err.message), JSON.stringify(bad));
    assert.throws(() => la.svd_vals(eye(4), {subset: bad}), err => /subset must be \[i0, i1\]/.test(err.message), JSON.stringify(bad));
    for (const fn of ['bidiag_svd', 'bidiag_svdvals'])
      assert.throws(() => la[fn](vec(1, 2, 3, 4), vec(1, 2, 3), {subset: bad}), err => /subset must be \[i0, i1\] with 0 <= i0 <= i1 <= K/.test(err.message), fn);
  }
  assert.throws(() => la.svd_decomp(eye(4), {subset: [0, 1], algo: 'jacobi'}), /subset is not available with algo 'jacobi'/);
  assert.throws(() => la.svd_decomp(eye(4), {subset: [0, 1], algo: 'qr'}), /algo must be/);
  // an NDArray has no axis of length 0 (the reference's constructor refuses it), so the JS layer refuses the empty subset
  assert.throws(() => la.svd_decomp(eye(4), {subset: [2, 2]}), /the subset \[2, 2\] is empty/);
  assert.throws(() => la.svd_vals(eye(4), {subset: [4, 4]}), /the subset \[4, 4\] is empty/);
  assert.throws(() => la.bidiag_svd(vec(1, 2), vec(1), {subset: [1, 1]}), /the subset \[1, 1\] is empty/);
  for (const fn of ['bidiag_svd', 'bidiag_svdvals']) {
    assert.throws(() => la[fn](vec(1, 2, 3), vec(1, 2, 3, 4)), /e must have the leading dimensions of d and len\(d\) - 1 or len\(d\) entries/, fn);
    assert.throws(() => la[fn](vec(1, 2, 3), null), /e must have the leading dimensions/, fn);
  }
  assert.throws(() => la.svd_vals(vec(1, 2, 3)), /A.ndim must be at least 2/);
  for (const k of ['svd_vals', 'bidiag_svd', 'bidiag_svdvals']) assert(typeof la[k] === 'function' && !Object.keys(la).includes(k), k);
}

if (mode === 'cpu') {
  argumentErrors();
  console.log('node svd subset cpu checks ok');
} else if (mode === 'gpu') {
  const cases = JSON.parse(fs.readFileSync(process.argv[3]));
  let n = 0;
  const host = x => la.to_host(x).data;
  for (const [name, c] of Object.entries(cases.dense)) {
    const shape = Int32Array.from(c.shape), nd_ = shape.length, M = shape[nd_ - 2], N = shape[nd_ - 1], k = c.subset[1] - c.subset[0];
    const data = Float64Array.from(c.A), A = new la.NDArray(shape, data), keep = Float64Array.from(data), opts = {subset: c.subset};
    const uW = Float64Array.from(c.U), sW = Float64Array.from(c.sv), vW = Float64Array.from(c.V), lead = Array.from(shape.subarray(0, nd_ - 2));
    const [U, sv, V] = la.svd_decomp(A, opts);
    assert(U instanceof la.NDArray && sv instanceof la.NDArray && V instanceof la.NDArray, name + ' host in, host out');
    assert.deepStrictEqual(Array.from(U.shape), lead.concat([M, k]), name); assert.deepStrictEqual(Array.from(sv.shape), lead.concat([k]), name);
    assert.deepStrictEqual(Array.from(V.shape), lead.concat([k, N]), name);
    assert(sameBits(U.data, uW) && sameBits(sv.data, sW) && sameBits(V.data, vW), name + ': other bits than the Python result');
    assert(sameBits(data, keep), name + ': A was written');
    assert(sameBits(la.svd_vals(A, opts).data, sW) && sameBits(la.svd_decomp(A, {subset: c.subset, algo: 'dc'})[1].data, sW), name + ': svd_vals has other bits');
    const Ad = la.to_device(A), [Ud, sd, Vd] = la.svd_decomp(Ad, opts), s2 = la.svd_vals(Ad, opts);
    assert(Ud instanceof la.DeviceNDArray && sd instanceof la.DeviceNDArray && Vd instanceof la.DeviceNDArray && s2 instanceof la.DeviceNDArray, name + ' device in, device out');
    assert(sameBits(host(Ud), uW) && sameBits(host(sd), sW) && sameBits(host(Vd), vW) && sameBits(host(s2), sW), name + ' device bits');
    assert(sameBits(host(Ad), keep), name + ': the device A was written');
    if (c.all) assert(sameBits(la.svd_vals(A).data, Float64Array.from(c.all)), name + ': svd_vals(A) has other bits');
    n++;
  }
  for (const [name, c] of Object.entries(cases.bidiag)) {
    const K = c.d.length, J = c.e.length + 1, k = c.subset[1] - c.subset[0], opts = {subset: c.subset};
    const d = vec(...c.d), e = c.e.length ? vec(...c.e) : null;
    const uW = Float64Array.from(c.U2), sW = Float64Array.from(c.sv), vW = Float64Array.from(c.V2);
    const [U2, sv, V2] = la.bidiag_svd(d, e, opts);
    assert.deepStrictEqual(Array.from(U2.shape), [K, k], name); assert.deepStrictEqual(Array.from(V2.shape), [k, J], name);
    assert(sameBits(U2.data, uW) && sameBits(sv.data, sW) && sameBits(V2.data, vW), name + ': other bits than the Python result');
    assert(sameBits(la.bidiag_svdvals(d, e, opts).data, sW), name + ': bidiag_svdvals has other bits');
    const dd = la.to_device(d), ed = e ? la.to_device(e) : null, [Ud, sd, Vd] = la.bidiag_svd(dd, ed, opts);
    assert(Ud instanceof la.DeviceNDArray, name + ' device in, device out');
    assert(sameBits(host(Ud), uW) && sameBits(host(sd), sW) && sameBits(host(Vd), vW) && sameBits(host(la.bidiag_svdvals(dd, ed, opts)), sW), name + ' device bits');
    if (c.all) assert(sameBits(la.bidiag_svdvals(d, e).data, Float64Array.from(c.all)), name + ': bidiag_svdvals(d, e) has other bits');
    n++;
  }
  argumentErrors();
  assert.throws(() => la.bidiag_svd(vec(1, NaN, 3), vec(1, 2), {subset: [0, 1]}), /d or e contains NaN or Infinity/);
  assert.throws(() => la.svd_vals(new la.NDArray(Int32Array.of(2, 2), Float64Array.of(1, 0, Infinity, 1))), /A contains NaN or Infinity/);
  console.log('node svd subset gpu checks ok', n);
} else throw new Error('mode');
