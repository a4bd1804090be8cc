'use strict';
/* Node-side checks of eigen_sym / eigenvals_sym with {algo: 'jacobi'} through the JS host and the N-API addon. Driven by
 * tests/test_node_eigsym_jacobi.py.
 *   node node_eigsym_jacobi_checks.js cpu                 (no GPU: the option's errors, the names stay non-enumerable)
 *   node node_eigsym_jacobi_checks.js gpu <cases.json>    (GPU: lambda and V of each case must be the bits of the numpy model of
 *                                                          tests/eigsym_jacobi_common.py, from host arrays and from DeviceNDArrays;
 *                                                          floats travel as hexadecimal bit patterns)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const NAMES = ['eigen_sym', 'eigenvals_sym'];
const sameBits = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const fromHex = hex => { const b = Buffer.from(hex, 'hex'); return new Float64Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength)); };
const mk = (shape, data) => new la.NDArray(Int32Array.from(shape), data);

if (mode === 'cpu') {
  for (const fn of NAMES) {
    assert(!Object.keys(la).includes(fn) && !Object.prototype.propertyIsEnumerable.call(la, fn), fn + ' must not be enumerable');
    for (const algo of ['qr', 'Jacobi', '', 0])
      assert.throws(() => la[fn](mk([2, 2], new Float64Array(4)), {algo}), err => err.message === `${fn}(S, {algo}): algo must be 'dc' or 'jacobi'.`, fn);
    for (const opts of [{algo: 'jacobi'}, {algo: 'dc'}, {}, undefined, null]) {
      assert.throws(() => la[fn](mk([3], Float64Array.of(1, 2, 3)), opts), err => err.message === `${fn}(S): S.ndim must be at least 2.`, fn);
      assert.throws(() => la[fn](mk([2, 3], new Float64Array(6)), opts), err => err.message === `${fn}(S): S must be quadratic.`, fn);
      assert.throws(() => la[fn](mk([2, 2], new Float32Array(4)), opts), err => err instanceof TypeError, fn + ' float32');
    }
  }
  console.log('node eigsym jacobi cpu checks ok');
} else if (mode === 'gpu') {
  const cases = JSON.parse(fs.readFileSync(process.argv[3]));
  let n = 0;
  for (const [name, c] of Object.entries(cases)) {
    const data = fromHex(c.S), lamM = fromHex(c.lam), VM = fromHex(c.V), keep = Float64Array.from(data), S = mk(c.shape, data);
    const [lam, V] = la.eigen_sym(S, {algo: 'jacobi'});
    assert(lam instanceof la.NDArray && V instanceof la.NDArray, name + ' host in, host out');
    assert.deepStrictEqual(Array.from(lam.shape), c.shape.slice(0, -1), name); assert.deepStrictEqual(Array.from(V.shape), c.shape, name);
    assert(sameBits(lam.data, lamM), name + ': lambda is not the model\'s');
    assert(sameBits(V.data, VM), name + ': V is not the model\'s');
    assert(sameBits(data, keep), name + ': S was written');
    assert(sameBits(la.eigenvals_sym(S, {algo: 'jacobi'}).data, lamM), name + ': eigenvals_sym has other bits');
    const Sd = la.to_device(S), [ld, Vd] = la.eigen_sym(Sd, {algo: 'jacobi'}), l2 = la.eigenvals_sym(Sd, {algo: 'jacobi'});
    assert(ld instanceof la.DeviceNDArray && Vd instanceof la.DeviceNDArray && l2 instanceof la.DeviceNDArray, name + ' device in, device out');
    assert(sameBits(la.to_host(ld).data, lamM) && sameBits(la.to_host(Vd).data, VM) && sameBits(la.to_host(l2).data, lamM), name + ' device bits');
    assert(sameBits(la.to_host(Sd).data, keep), name + ': the device S was written');
    // {algo: 'dc'} and no option are the default route
    const [l0, V0] = la.eigen_sym(S), [l1, V1] = la.eigen_sym(S, {algo: 'dc'});
    assert(sameBits(l0.data, l1.data) && sameBits(V0.data, V1.data) && sameBits(la.eigenvals_sym(S, {algo: 'dc'}).data, l0.data), name + ': dc');
    n++;
  }
  const bad = mk([2, 2], Float64Array.of(1, 0, NaN, 1));
  for (const fn of NAMES) assert.throws(() => la[fn](bad, {algo: 'jacobi'}), /eigen_sym\(S\): S contains NaN or Infinity in its lower triangle\./);
  assert.throws(() => la.eigen_sym(mk([129, 129], new Float64Array(129 * 129)), {algo: 'jacobi'}), /N <= 128/);
  const [lam] = la.eigen_sym(mk([2, 2], Float64Array.of(1, 0.5, 0.5, 1)), {algo: 'jacobi'});     // usable after the errors
  assert.deepStrictEqual(Array.from(lam.data), [1.5, 0.5]);
  console.log('node eigsym jacobi gpu checks ok', n);
} else throw new Error('mode');
