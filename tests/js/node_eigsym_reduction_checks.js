'use strict';
/* Node-side checks of eigen_sym / eigenvals_sym with opts.reduction through the JS host and the N-API addon. Driven by
 * tests/test_node_eigsym_reduction.py.
 *   node node_eigsym_reduction_checks.js cpu                 (no GPU: the argument errors of opts.reduction)
 *   node node_eigsym_reduction_checks.js gpu <cases.json>    (GPU: host arrays and DeviceNDArrays give the bits of the Python result)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const NAMES = ['eigen_sym', 'eigenvals_sym'];
const sameBits = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const eye = N => { const d = new Float64Array(N * N); for (let i = 0; i < N; i++) d[i * N + i] = 1; return new la.NDArray(Int32Array.of(N, N), d); };

function reductionErrors() {
  for (const fn of NAMES) {
    for (const bad of ['tri', 'sytrd', 1, true, ['tridiag']])
      assert.throws(() => la[fn](eye(4), {reduction: bad}), err => /reduction must be 'hessenberg' or 'tridiag'/.test(err.message), `${fn} ${JSON.stringify(bad)}`);
    assert.throws(() => la[fn](eye(4), {reduction: 'tridiag', algo: 'jacobi'}), /reduction is not available with algo 'jacobi'/, fn);
    assert.throws(() => la[fn](eye(4), {reduction: 'tridiag', subset: [3, 2]}), /subset must be/, fn);
  }
}

if (mode === 'cpu') {
  reductionErrors();
  console.log('node eigsym reduction cpu checks ok');
} else if (mode === 'gpu') {
  const cases = JSON.parse(fs.readFileSync(process.argv[3]));
  let n = 0;
  for (const [name, c] of Object.entries(cases)) {
    const shape = Int32Array.from(c.shape), N = shape[shape.length - 1], k = c.subset ? c.subset[1] - c.subset[0] : N;
    const data = Float64Array.from(c.S), S = new la.NDArray(shape, data), keep = Float64Array.from(data);
    const opts = c.subset ? {reduction: 'tridiag', subset: c.subset} : {reduction: 'tridiag'};
    const lamWant = Float64Array.from(c.lam), vWant = Float64Array.from(c.V), lead = Array.from(shape.subarray(0, shape.length - 2));
    const [lam, V] = la.eigen_sym(S, opts);
    assert(lam instanceof la.NDArray && V instanceof la.NDArray, name + ' host in, host out');
    assert.deepStrictEqual(Array.from(lam.shape), lead.concat([k]), name); assert.deepStrictEqual(Array.from(V.shape), lead.concat([N, k]), name);
    assert(sameBits(lam.data, lamWant) && sameBits(V.data, vWant), name + ': other bits than the Python result');
    assert(sameBits(data, keep), name + ': S was written');
    assert(sameBits(la.eigenvals_sym(S, opts).data, lamWant), name + ': eigenvals_sym has other bits');
    const Sd = la.to_device(S), [ld, Vd] = la.eigen_sym(Sd, opts), l2 = la.eigenvals_sym(Sd, opts);
    assert(ld instanceof la.DeviceNDArray && Vd instanceof la.DeviceNDArray && l2 instanceof la.DeviceNDArray, name + ' device in, device out');
    assert.deepStrictEqual(Array.from(Vd.shape), lead.concat([N, k]), name);
    assert(sameBits(la.to_host(ld).data, lamWant) && sameBits(la.to_host(Vd).data, vWant) && sameBits(la.to_host(l2).data, lamWant), name + ' device bits');
    assert(sameBits(la.to_host(Sd).data, keep), name + ': the device S was written');
    // 'hessenberg' is the default route
    if (c.lam0) assert(sameBits(la.eigenvals_sym(S, {reduction: 'hessenberg'}).data, Float64Array.from(c.lam0)), name + ': hessenberg is not the default');
    n++;
  }
  reductionErrors();
  const bad = new la.NDArray(Int32Array.of(2, 2), Float64Array.of(1, 0, NaN, 1));
  assert.throws(() => la.eigen_sym(bad, {reduction: 'tridiag'}), /NaN or Infinity in its lower triangle/);
  console.log('node eigsym reduction gpu checks ok', n);
} else throw new Error('mode');
